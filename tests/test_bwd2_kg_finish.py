"""The KG rows' query-gradient chain of the row-space backward, in both of its forms (csrc/fused_rows.hip bwd2_kernel, csrc/gemm16.hip
GF_KGQ): finished by the last-arriving block of bwd2 (dG = dGpart + dQ2.Wq2, then dG^T.KG in the weight-gradient launch), or left to
the weight-gradient launch, which takes  dGpart^T.KG + Wq2^T.(dQ2^T.KG)  and the in-projection's q rows from the fp32 dQ2 sums.
One training step (bf16, dropout 0.3) per form against the oracle in its bf16-operand mode, at the bounds of
test_hip_fused.py::_training_step_shape_envelope and, since the q rows this is about are ~1e-3 of their packed tensor's norm, block by
block (helpers.assert_attention_grad_blocks_close); the two forms' q rows within twice that bound of each other, each being within
it of the same oracle step.  The identity itself is checked on the CPU."""
import numpy as np
import pytest
import torch

from helpers import (ATTN_BLOCK_BOUND, assert_attention_grad_blocks_close, assert_close, bf16_oracle, oracle_step_at_relu_thresholds,
                     single_column_attentions)
from oracle import fusion_oracle as FO
from oracle import params as OP

DEFER_MAX_TK = 512            # csrc/fused_rows.h, FUSED_BWD2_DEFER_MAX_TK: by size the weight-gradient launch takes the chain up to here


def test_deferred_weight_gradient_identity_f64():
    """dG = dGpart + dQ2.Wq2  =>  dG^T.KG = dGpart^T.KG + Wq2^T.(dQ2^T.KG)  and  colsum(dG) = colsum(dGpart) + Wq2^T.colsum(dQ2),
    in float64 on random operands (TK = 208 rows, as at B = 16): a transpose in the wrong place does not survive this."""
    rs = np.random.RandomState(3)
    TK, H, D = 208, 256, 128
    dGpart, dQ2 = rs.standard_normal((TK, H)), rs.standard_normal((TK, H))
    Wq2, KG = rs.standard_normal((H, H)), rs.standard_normal((TK, D))      # q2 = g.Wq2^T: Wq2 is [out j][in i]
    dG = dGpart + dQ2 @ Wq2
    Mq = dQ2.T @ KG
    dW = dGpart.T @ KG + Wq2.T @ Mq
    db = dGpart.sum(0) + Wq2.T @ dQ2.sum(0)
    assert np.abs(dW - dG.T @ KG).max() <= 1e-12 * np.abs(dG.T @ KG).max()
    assert np.abs(db - dG.sum(0)).max() <= 1e-12 * np.abs(dG.sum(0)).max()
    # the K-sliced form the blocks run: output rows 64 q .., K slice 64 c .. of Wq2^T.Mq, summed over c
    dW2 = dGpart.T @ KG
    for q in range(4):
        for c in range(4):
            dW2[64 * q:64 * q + 64] += Wq2[64 * c:64 * c + 64, 64 * q:64 * q + 64].T @ Mq[64 * c:64 * c + 64]
    assert np.abs(dW2 - dG.T @ KG).max() <= 1e-12 * np.abs(dG.T @ KG).max()


def _opt(name, value):
    from camouflage_multimodal_amd import _lib
    _lib.check(_lib.lib().camo_debug_set_option(name.encode(), value), "camo_debug_set_option")


@pytest.fixture
def exp_opt():
    yield lambda v: _opt("exp", v)
    _opt("exp", 0)


def _rel(a, b):
    a = a.astype(np.float64); b = b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


CASES = [
    ([1], 13),                                            # one tile with one row
    ([33, 32, 64], 16),                                   # partial, exact and double tiles; no padding rows in the 16-row images
    ([33, 32, 64], 1),
    ([40 + 2 * i for i in range(16)], 13),                # the headline's plan: one-launch tail, its weight gradients in bwd1
    ([9, 40, 33, 1, 64, 17, 31, 2, 48, 5, 32, 20, 65, 3, 12, 7, 26], 13),     # B = 17: the grouped tail beside it
    ([3 + (5 * i) % 11 for i in range(32)], 16),          # B Nk = 512: the last size the weight-gradient launch takes by size
    ([3 + (5 * i) % 11 for i in range(33)], 16),          # B Nk = 528: by size the arrival protocol again
]


@pytest.mark.gpu
@pytest.mark.parametrize("nrs,nk", CASES)
def test_kg_query_gradient_chain_both_forms(nrs, nk, exp_opt):
    from camouflage_multimodal_amd import _lib
    from test_hip_parity import make_model, outs6, t2n
    pseed, dseed = 6, 1234
    cfg = OP.full_cfg()
    m = make_model(cfg, pseed, "bf16").train()
    eng = m._engine
    B = len(nrs)
    rgl = [OP.make_rg(n, 128, seed=300 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, 128, seed=400 + i) for i in range(B)])
    y, e, s = OP.make_labels(B, seed=21)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    g = eng.ensure_flat_grads(attach=True)
    timeouts0 = _lib.tail_timeouts()
    runs = {}
    for name, exp in (("by size", 0), ("arrival protocol in bwd2", 32), ("weight-gradient launch", 64)):
        exp_opt(exp)
        g.zero_()
        outs, terms, _ = eng.train_raw(batch, eng.workspace(batch, private=True), torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s),
                                       True, dseed, eng._gtab)
        torch.cuda.synchronize()
        runs[name] = (t2n(outs).copy(), t2n(terms).copy(), {k: t2n(p.grad).copy() for k, p in m.named_parameters()})
    exp_opt(0)
    assert _lib.tail_timeouts() == timeouts0
    old, new = runs["arrival protocol in bwd2"], runs["weight-gradient launch"]
    assert_close(new[0], old[0], 1e-6, 0, "forward outputs of the two forms")
    assert_close(runs["by size"][0], old[0], 1e-6, 0, "forward outputs, form chosen by size")
    H = 256
    between = {}
    for k, sl in (("kg_proj.weight", slice(None)), ("kg_proj.bias", slice(None)), ("cross_attn_kg2rg.in_proj_weight", slice(0, H)), ("cross_attn_kg2rg.in_proj_bias", slice(0, H))):
        name = [n for n in old[2] if n.endswith(k)]
        assert len(name) == 1, (k, sorted(old[2]))
        between[k] = _rel(new[2][name[0]][sl], old[2][name[0]][sl])
        print(f"nrs={nrs[:4]}.. nk={nk}: {k}{' q rows' if sl != slice(None) else ''}: relative difference between the forms {between[k]:.2e}")
    # by size the form follows B Nk alone (row space here: far below 10 240 packed rows); the chosen form sums the same values in the same
    # order as the forced one except for the fp32 atomics' arrival order
    same = new if B * nk <= DEFER_MAX_TK else old
    for k in same[2]:
        scale = max(float(np.abs(same[2][k]).max()), 1e-8)
        assert float(np.abs(runs["by size"][2][k] - same[2][k]).max()) <= 4e-3 * scale + 2e-7, ("the form chosen by size", k)
    grads0 = runs["by size"][2]
    ref, near, flipped = oracle_step_at_relu_thresholds(
        lambda: bf16_oracle(cfg, OP.make_params(cfg, pseed), nrs, False),
        lambda o: FO.train_step(o, FO.AdamW(o.p), rgl, kg, y, e, s, training=True, seed=dseed), grads0)
    if near:
        print("tail units at the ReLU threshold (site, sample, unit, pre-activation):", near, "taken flipped:", flipped)
    den = sum(float((ref["raw_grads"][k].astype(np.float64) ** 2).sum()) for k in grads0)
    for name, (outs, terms, grads) in runs.items():
        assert np.isfinite(outs).all() and all(np.isfinite(v).all() for v in grads.values()), name
        assert_close(outs, outs6(ref["outs"]), 5e-4, 0, f"{name}: outputs vs the bf16-operand oracle")
        assert_close(terms, ref["loss_terms"], 2e-3, 1e-3, f"{name}: loss terms")
        num = sum(float(((grads[k].astype(np.float64) - ref["raw_grads"][k]) ** 2).sum()) for k in grads)
        per = sorted(((_rel(grads[k], ref["raw_grads"][k]), k) for k in grads if (ref["raw_grads"][k].astype(np.float64) ** 2).sum() > 1e-6 * den), reverse=True)
        total = float(np.sqrt(num / den))
        print(f"   {name}: global relative gradient error vs the bf16-operand oracle {total:.5f}; worst {per[0][1]} {per[0][0]:.4f}")
        assert total < 2e-3, (name, total, per[:4])
        assert per[0][0] < 1e-2, (name, per[:4])
        assert_attention_grad_blocks_close(grads, ref["raw_grads"], what=f"nrs={nrs[:4]}.. nk={nk}, {name}",
                                           single_column=single_column_attentions(nrs, nk))
    # (one-node samples only: the KG->RG softmax has one column, these q rows are zero in exact arithmetic and both forms hold rounding noise)
    for k in () if "kg2rg" in single_column_attentions(nrs, nk) else ("cross_attn_kg2rg.in_proj_weight", "cross_attn_kg2rg.in_proj_bias"):
        assert between[k] <= 2 * ATTN_BLOCK_BOUND, f"{k} q rows: the two forms differ by {between[k]:.2e} of the block's norm"
