"""The 32-row tile kernels (csrc/fused_rows.hip) where their hoisted, clamped loads can go wrong.  Needs an MI355X.

The kernels load what their epilogues need -- parameter vectors into an LDS table, this lane's residual / dU / xhat / O2 row into
registers or LDS -- at block start, with the row index clamped into the tile.  The shapes here put a sample of one row (a tile of
one row), 31, 32, 33 and 65 rows (a full tile, one-row and two-tile remainders) into one batch, with Nk = 13 (three padded KG rows)
and Nk = 16 (none), B = 1, dropout 0.3 and 0; a training call and an inference call are held to the oracle with the bounds of
test_hip_fused.py's stage and envelope tests, and one training call runs in a workspace pre-filled with 0x7F bytes (bf16 3.4e38,
fp32 3.4e38: any value read from past a tensor's last row poisons what is computed from it)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_attention_grad_blocks_close, assert_close, bf16_oracle, oracle_step_at_relu_thresholds, single_column_attentions
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_hip_parity import make_model, outs6, t2n

pytestmark = pytest.mark.gpu

NRS = [1, 31, 32, 33, 65]
CASES = [(NRS, 13, 0.3), (NRS, 16, 0.3), (NRS, 13, 0.0), ([33], 13, 0.3), ([1], 16, 0.0)]


def _opt(name, value):
    from camouflage_multimodal_amd import _lib
    _lib.check(_lib.lib().camo_debug_set_option(name.encode(), value), "camo_debug_set_option")


@pytest.fixture
def tiles32():
    _opt("wide2", 0); _opt("wide2_bwd", 0); _opt("fused_rt", 0)      # the 32-row tile kernels, whatever the size rules would pick
    yield
    _opt("wide2", -1); _opt("wide2_bwd", -1); _opt("fused_rt", -1)


def _inputs(nrs, nk):
    rgl = [OP.make_rg(n, 128, seed=500 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, 128, seed=600 + i) for i in range(len(nrs))])
    return rgl, kg


def _train_and_check(nrs, nk, drop, guard):
    cfg = OP.full_cfg(dict(dropout=drop))
    pseed, dseed = 6, 4321
    m = make_model(cfg, pseed, "bf16").train()
    eng = m._engine
    rgl, kg = _inputs(nrs, nk)
    y, e, s = OP.make_labels(len(nrs), seed=31)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    ws = eng.workspace(batch, private=True)
    if guard:
        ws.fill_(0x7F)
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    outs, terms, _ = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, dseed, eng._gtab)
    torch.cuda.synchronize()
    grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    assert np.isfinite(t2n(outs)).all() and all(np.isfinite(v).all() for v in grads.values())
    ref, near, flipped = oracle_step_at_relu_thresholds(
        lambda: bf16_oracle(cfg, OP.make_params(cfg, pseed), nrs, False),
        lambda o: FO.train_step(o, FO.AdamW(o.p), rgl, kg, y, e, s, training=True, seed=dseed), grads)
    if near:
        print("tail units at the ReLU threshold:", near, "taken flipped:", flipped)
    assert_close(t2n(outs), outs6(ref["outs"]), 5e-4, 0, "outputs vs the bf16-operand oracle")
    assert_close(t2n(terms), ref["loss_terms"], 2e-3, 1e-3, "loss terms")
    rg_ = ref["raw_grads"]
    den = sum(float((rg_[k].astype(np.float64) ** 2).sum()) for k in grads)
    num = sum(float(((grads[k].astype(np.float64) - rg_[k]) ** 2).sum()) for k in grads)
    per = sorted(((float(np.sqrt(((grads[k].astype(np.float64) - rg_[k]) ** 2).sum() / max((rg_[k].astype(np.float64) ** 2).sum(), 1e-30))), k)
                  for k in grads if (rg_[k].astype(np.float64) ** 2).sum() > 1e-6 * den), reverse=True)
    total = float(np.sqrt(num / den))
    print(f"nrs={nrs} nk={nk} dropout={drop} guard={guard}: global relative gradient error {total:.5f}; worst {per[0][1]} {per[0][0]:.4f}")
    assert total < 2e-3, (total, per[:4])
    assert per[0][0] < 1e-2, per[:4]
    assert_attention_grad_blocks_close(grads, rg_, what=f"nrs={nrs} nk={nk}", single_column=single_column_attentions(nrs, nk))
    return eng, batch, ws


@pytest.mark.parametrize("nrs,nk,drop", CASES)
def test_training_call_on_ragged_tiles(nrs, nk, drop, tiles32):
    _train_and_check(nrs, nk, drop, guard=False)


@pytest.mark.parametrize("nrs,nk,drop", CASES)
def test_inference_call_on_ragged_tiles(nrs, nk, drop, tiles32):
    cfg = OP.full_cfg(dict(dropout=drop))
    m = make_model(cfg, 2, "bf16").eval()
    rgl, kg = _inputs(nrs, nk)
    ref, _ = FO.FusionOracle(cfg, OP.make_params(cfg, 2)).forward_list(rgl, kg)
    with torch.no_grad():
        o = m.forward_packed(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    got = np.concatenate([t2n(v) for v in o], axis=1)
    assert np.isfinite(got).all()
    assert_close(got, outs6(ref), 1e-3, 0, f"nrs={nrs} nk={nk}")


def test_guard_rows_behind_the_last_row_stay_out_of_the_results(tiles32):
    """The whole workspace holds 0x7F bytes before the call, so the rows behind the last row of dU16, dR16, O2_16 and R16 do: the
    call's results still meet the oracle (no poisoned value was used), and those rows come out either untouched or cleared (the
    pad rows of a weight-gradient operand are cleared by the step): nothing computed was written past a tensor's end."""
    from camouflage_multimodal_amd import _lib
    nk = 13
    eng, batch, ws = _train_and_check(NRS, nk, 0.3, guard=True)
    T, K = sum(NRS), len(NRS) * nk
    for name, rows in (("dU16", T), ("dR16", T), ("R16", T), ("O2_16", K)):
        off = _lib.lib().camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
        assert off >= 0, name
        row = ws[off + 2 * 256 * rows: off + 2 * 256 * (rows + 1)].cpu().numpy()
        assert (row == 0x7F).all() or (row == 0).all(), f"{name}: the row behind the last one holds computed values"
