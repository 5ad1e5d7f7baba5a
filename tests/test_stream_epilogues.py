"""The 32-row tile kernels (csrc/fused_rows.hip) where the tile-major walk and the early dropout draws can go wrong.  Needs an MI355X.

back_kernel's FFN and front_kernel's in-projections walk their weight stream tile by tile and run tile t's epilogue in the gaps of
tile t + 1's stream; the attention kernels draw their dropout keep bits at block start, from indices alone.  A wrong register-to-row
mapping, a wrong index or a tile's epilogue run on the wrong accumulator shows in the saved FFN masks EXACTLY (a bit set where the
oracle's draw drops the element cannot come from rounding), so they are checked bit by bit; the rest of the call is held to the
oracle with the bounds of test_tile_epilogues.py.  Shapes: samples of 1, 31, 32, 33, 65 and 129 rows in one batch (a one-row tile, a
full tile, one-row and two-tile remainders; 65 and 129 rows: a KG split with a single valid key behind one and two full splits),
Nk = 13 (the skipped register groups of the KG tile) and 16, dropout 0.3, 0.9 and 0, two dropout seeds, B = 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_attention_grad_blocks_close, assert_close, bf16_oracle, oracle_step_at_relu_thresholds, single_column_attentions
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_hip_parity import make_model, outs6, t2n
from test_tile_epilogues import tiles32  # noqa: F401  (fixture: the 32-row tile kernels, whatever the size rules would pick)

pytestmark = pytest.mark.gpu

NRS = [1, 31, 32, 33, 65, 129]
PSEED = 6
# (nrs, nk, dropout, dropout seed, workspace pre-filled with 0x7F)
TRAIN_CASES = [(NRS, 13, 0.3, 4321, False), (NRS, 16, 0.3, 4321, True), (NRS, 13, 0.9, 4321, False), (NRS, 13, 0.0, 4321, False),
               (NRS, 13, 0.3, 977, False), ([33], 13, 0.3, 4321, False), ([129], 16, 0.9, 977, False)]
INFER_CASES = [(NRS, 13), (NRS, 16), ([33], 13), ([129], 16)]
H_NEAR = 2e-2           # test_hip_fused.py's stage test: an FFN activation closer to 0 than this may land on either side of the ReLU
MAX_NEAR = 0.05         # at most this fraction of a mask's elements may be left out as too close to 0

# what no float atomic feeds (bytes per row; rows: T = RG rows, K = B * Nk)
EXACT = (("Q16", "T", 512), ("KV16", "K", 1024), ("R16", "T", 512), ("Q2_16", "K", 512), ("KV2_16", "T", 1024), ("O16", "T", 512),
         ("Y16", "T", 512), ("XH16", "T", 512), ("mask1", "T", 64), ("mask2", "K", 64), ("rstd1", "T", 4), ("rstd2", "K", 4))


def _inputs(nrs, nk):
    rgl = [OP.make_rg(n, 128, seed=500 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, 128, seed=600 + i) for i in range(len(nrs))])
    return rgl, kg


def _ws_bytes(eng, batch, ws, name, nbytes):
    from camouflage_multimodal_amd import _lib
    off = _lib.lib().camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
    assert off >= 0, name
    return ws[off:off + nbytes].cpu().numpy().copy()


def _train_call(m, nrs, nk, dseed, fill):
    eng = m._engine
    rgl, kg = _inputs(nrs, nk)
    y, e, s = OP.make_labels(len(nrs), seed=31)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    ws = eng.workspace(batch, private=True)
    ws.fill_(fill)
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    outs, terms, _ = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, dseed, eng._gtab)
    torch.cuda.synchronize()
    return eng, batch, ws, outs, terms


def _mask_bits(eng, batch, ws, name, rows):
    words = _ws_bytes(eng, batch, ws, name, 4 * rows * 16).view(np.uint32).reshape(rows, 16)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(rows, 512).astype(bool)


def _oracle_masks(cfg, nrs, nk, drop, dseed):
    """Per stream: (the bf16-operand oracle's FFN pre-activation [rows, 512], the oracle's keep draw [rows, 512]) -- oracle alone."""
    prm = OP.make_params(cfg, PSEED)
    rgl, kg = _inputs(nrs, nk)
    _, caches = bf16_oracle(cfg, prm, nrs, False).forward_list(rgl, kg, training=True, seed=dseed)
    out = {}
    for name, ykey, wname, site in (("mask1", "Y", "fusion.ffn_rg.0", FO.SITE_FFN_RG), ("mask2", "Y2", "fusion.ffn_kg.0", FO.SITE_FFN_KG)):
        pre = np.concatenate([FO._linear(FO.bf16_round(c[ykey]), FO.bf16_round(prm[wname + ".weight"]), prm[wname + ".bias"]) for c in caches])
        idx = np.arange(pre.size, dtype=np.uint64).reshape(pre.shape)        # element (row, unit) of the packed stream: row * 512 + unit
        keep = FO.dropout_keep(dseed, site, idx, drop) if drop > 0 else np.ones(pre.shape, bool)
        out[name] = (pre, keep)
    return out


@pytest.mark.parametrize("nrs,nk,drop,dseed,guard", TRAIN_CASES)
def test_training_call_and_saved_masks(nrs, nk, drop, dseed, guard, tiles32):  # noqa: F811
    cfg = OP.full_cfg(dict(dropout=drop))
    m = make_model(cfg, PSEED, "bf16").train()
    eng, batch, ws, outs, terms = _train_call(m, nrs, nk, dseed, 0x7F if guard else 0)
    # ---- the saved FFN masks, bit by bit
    _assert_masks(eng, batch, ws, cfg, nrs, nk, drop, dseed)
    # ---- the call against the oracle (bounds of test_tile_epilogues.py)
    rgl, kg = _inputs(nrs, nk)
    y, e, s = OP.make_labels(len(nrs), seed=31)
    grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    assert np.isfinite(t2n(outs)).all() and all(np.isfinite(v).all() for v in grads.values())
    ref, near_units, flipped = oracle_step_at_relu_thresholds(
        lambda: bf16_oracle(cfg, OP.make_params(cfg, PSEED), nrs, False),
        lambda o: FO.train_step(o, FO.AdamW(o.p), rgl, kg, y, e, s, training=True, seed=dseed), grads)
    if near_units:
        print("tail units at the ReLU threshold:", near_units, "taken flipped:", flipped)
    assert_close(t2n(outs), outs6(ref["outs"]), 5e-4, 0, "outputs vs the bf16-operand oracle")
    assert_close(t2n(terms), ref["loss_terms"], 2e-3, 1e-3, "loss terms")
    rg_ = ref["raw_grads"]
    sq = lambda a: float((np.asarray(a, np.float64) ** 2).sum())
    den = sum(sq(rg_[k]) for k in grads)
    total = float(np.sqrt(sum(sq(grads[k].astype(np.float64) - rg_[k]) for k in grads) / den))
    per = sorted(((float(np.sqrt(sq(grads[k].astype(np.float64) - rg_[k]) / max(sq(rg_[k]), 1e-30))), k)
                  for k in grads if sq(rg_[k]) > 1e-6 * den), reverse=True)
    print(f"nrs={nrs} nk={nk} dropout={drop} seed={dseed} guard={guard}: global relative gradient error {total:.5f}; worst {per[0][1]} {per[0][0]:.4f}")
    assert total < 2e-3, (total, per[:4])
    assert per[0][0] < 1e-2, per[:4]
    assert_attention_grad_blocks_close(grads, rg_, what=f"nrs={nrs} nk={nk}", single_column=single_column_attentions(nrs, nk))


def _assert_masks(eng, batch, ws, cfg, nrs, nk, drop, dseed):
    for name, (pre, keep) in _oracle_masks(cfg, nrs, nk, drop, dseed).items():
        bits = _mask_bits(eng, batch, ws, name, pre.shape[0])
        wrong_draw = bits & ~keep
        assert not wrong_draw.any(), (f"{name}: {int(wrong_draw.sum())} bits set where the draw drops the element, first at "
                                      f"(row, unit) {tuple(np.argwhere(wrong_draw)[0])}")
        near = np.abs(pre) < H_NEAR
        print(f"{name} nrs={nrs[:6]}{'...' if len(nrs) > 6 else ''} nk={nk} dropout={drop} seed={dseed}: {near.mean():.4f} of the elements "
              f"within {H_NEAR} of the ReLU threshold")
        assert near.mean() <= MAX_NEAR, (name, float(near.mean()))
        bad = (bits != ((pre > 0) & keep)) & ~near
        assert not bad.any(), f"{name}: {int(bad.sum())} wrong bits away from the threshold, first at (row, unit) {tuple(np.argwhere(bad)[0])}"


def test_saved_masks_past_two_blocks_per_cu(tiles32):  # noqa: F811
    """A launch of more than 512 blocks takes back_kernel's three-blocks-per-CU instantiation (its own LDS layout and register budget):
    264 samples of 1, 31, 32 and 33 rows = 264 KG blocks + 264 RG tiles.  The masks, bit by bit."""
    nrs, nk, drop, dseed = [1, 31, 32, 33] * 66, 13, 0.3, 4321
    cfg = OP.full_cfg(dict(dropout=drop))
    m = make_model(cfg, PSEED, "bf16").train()
    eng, batch, ws, outs, _ = _train_call(m, nrs, nk, dseed, 0)
    assert np.isfinite(t2n(outs)).all()
    _assert_masks(eng, batch, ws, cfg, nrs, nk, drop, dseed)


def test_same_seed_calls_are_byte_identical_where_no_atomic_feeds(tiles32):  # noqa: F811
    """Two calls with one seed: every saved tensor no float atomic feeds is byte-identical (a race on a deferred store or an LDS tile
    shows here); a call with another seed differs in both masks."""
    nk, drop = 13, 0.3
    cfg = OP.full_cfg(dict(dropout=drop))
    m = make_model(cfg, PSEED, "bf16").train()
    T, K = sum(NRS), len(NRS) * nk
    snaps = []
    for dseed in (4321, 4321, 977):
        eng, batch, ws, _, _ = _train_call(m, NRS, nk, dseed, 0)
        snap = {name: _ws_bytes(eng, batch, ws, name, per_row * (T if rows == "T" else K)) for name, rows, per_row in EXACT}
        snap["lse2"] = _ws_bytes(eng, batch, ws, "lse2", len(NRS) * 8 * 16 * 2 * 4)
        snaps.append(snap)
    for name in snaps[0]:
        assert snaps[0][name].any(), f"{name}: nothing was saved"
        assert np.array_equal(snaps[0][name], snaps[1][name]), f"{name}: two calls with one seed differ"
    for name in ("mask1", "mask2"):
        assert not np.array_equal(snaps[0][name], snaps[2][name]), f"{name}: the same mask under two seeds"


@pytest.mark.parametrize("nrs,nk", INFER_CASES)
def test_inference_call(nrs, nk, tiles32):  # noqa: F811
    cfg = OP.full_cfg(dict(dropout=0.0))
    m = make_model(cfg, 2, "bf16").eval()
    rgl, kg = _inputs(nrs, nk)
    ref, _ = FO.FusionOracle(cfg, OP.make_params(cfg, 2)).forward_list(rgl, kg)
    with torch.no_grad():
        o = m.forward_packed(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    got = np.concatenate([t2n(v) for v in o], axis=1)
    assert np.isfinite(got).all()
    assert_close(got, outs6(ref), 1e-3, 0, f"nrs={nrs} nk={nk}")
