"""The query and key weight gradients of both attentions, block by block.

Each attention keeps its q, k and v rows in one parameter (``in_proj_weight`` [3H, H], ``in_proj_bias`` [3H]), and at
initialisation-scale parameters the v rows carry that tensor's gradient: a q or k block is ~2e-3 of its norm.  The bf16 training
tests hold gradients per whole tensor (global relative L2 error < 2e-3, every tensor that carries weight < 1e-2), so a q or k block
that is zero, negated, doubled or has two heads exchanged passes all of them.  helpers.assert_attention_grad_blocks_close holds
the blocks and their heads to the oracle on their own norms.

CPU part: the shares that make the per-tensor bounds blind, and that five corruptions of the oracle's own gradients pass the
per-tensor acceptance and fail the block check.  GPU part (needs an MI355X): one bf16 training step with dropout 0.3 at SHARP
parameters (helpers._sharp_params: q and k rows x 12, attention maps far from uniform, so the softmax backward P o (dP - delta) runs
with a non-uniform P) on every form of the backward, against the oracle in its bf16-operand mode: outputs, loss terms, the two
tensor-level bounds and the block check."""
import functools

import numpy as np
import pytest

from helpers import (ATTN_BLOCK_BOUND, ATTN_BLOCK_CAP, QK_GAIN, _log_spread, _sharp_params, assert_attention_grad_blocks_close,
                     assert_close, attention_grad_blocks, bf16_oracle, oracle_step_at_relu_thresholds, single_column_attentions)
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_bwd2_kg_finish import CASES as KG_FINISH_CASES

NRS6 = [33, 31, 1, 2, 530, 96]
HEADLINE_PLAN = [40 + 2 * i for i in range(16)]
B17 = next(n for n, _ in KG_FINISH_CASES if len(n) == 17)
PSEED, DSEED = 6, 1234
RG2KG_W, KG2RG_W = "fusion.cross_attn_rg2kg.in_proj_weight", "fusion.cross_attn_kg2rg.in_proj_weight"
RG2KG_B = "fusion.cross_attn_rg2kg.in_proj_bias"


def _norm(x):
    return float(np.sqrt((np.asarray(x, np.float64) ** 2).sum()))


@functools.lru_cache(maxsize=None)
def _inputs(nrs, nk):
    """The inputs of test_hip_fused.py::_training_step_shape_envelope for this shape (shared, never written to)."""
    B = len(nrs)
    rgl = [OP.make_rg(n, 128, seed=300 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, 128, seed=400 + i) for i in range(B)])
    return (rgl, kg) + tuple(OP.make_labels(B, seed=21))


def _params(cfg, sharp, pseed=PSEED, gain=QK_GAIN):
    return _sharp_params(cfg, pseed, gain) if sharp else OP.make_params(cfg, pseed)       # (a fresh copy: a train step updates it in place)


@functools.lru_cache(maxsize=None)
def _oracle_step(sharp, bf16, nrs=tuple(NRS6), nk=13, gain=QK_GAIN):
    """raw_grads of one training step (dropout 0.3) of the oracle, f32 or bf16-operand mode; computed once per process."""
    cfg = OP.full_cfg()
    assert cfg["dropout"] == 0.3
    rgl, kg, y, e, s = _inputs(nrs, nk)
    orc = FO.FusionOracle(cfg, _params(cfg, sharp, gain=gain), bf16_operands=bf16)
    return FO.train_step(orc, FO.AdamW(orc.p), rgl, kg, y, e, s, training=True, seed=DSEED)["raw_grads"]


def _tensor_acceptance(got, ref):
    """The two bounds of test_hip_fused.py::_training_step_shape_envelope, recomputed exactly as there: -> (global relative error,
    [(relative error, tensor)] over the tensors with more than 1e-6 of the squared global norm, worst first)."""
    den = sum(float((ref[k].astype(np.float64) ** 2).sum()) for k in got)
    num = sum(float(((got[k].astype(np.float64) - ref[k]) ** 2).sum()) for k in got)
    per = sorted(((float(np.sqrt(((got[k].astype(np.float64) - ref[k]) ** 2).sum() / max((ref[k].astype(np.float64) ** 2).sum(), 1e-30))), k)
                  for k in got if (ref[k].astype(np.float64) ** 2).sum() > 1e-6 * den), reverse=True)
    return float(np.sqrt(num / den)), per


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_q_and_k_blocks_carry_under_a_percent_of_their_tensor():
    """The reason the block check exists: in the f32 oracle's step at OP.make_params (seed 6, dropout 0.3, nrs NRS6, Nk 13) the q and
    k weight blocks of both attentions carry < 1e-2 of their packed tensor's norm (1.7e-3 / 2.1e-3 and 7.2e-4 / 8.1e-4), and scaling
    the q / k projections by 12 leaves the KG->RG q block at 9.7e-3: a zeroed block there is still inside the per-tensor 1e-2."""
    H = 256
    g = _oracle_step(False, False)
    for k in (RG2KG_W, KG2RG_W):
        for i, r in enumerate("qk"):
            share = _norm(g[k][i * H:(i + 1) * H]) / _norm(g[k])
            print(f"{k} {r} rows: {share:.2e} of the tensor's norm")
            assert 0 < share < 1e-2, (k, r, share)
    g12 = _oracle_step(True, False)
    share = _norm(g12[KG2RG_W][:H]) / _norm(g12[KG2RG_W])
    print(f"gain {QK_GAIN}: {KG2RG_W} q rows: {share:.2e} of the tensor's norm")
    assert 0 < share < 1e-2, share


def _corruptions(ref):
    H, dh = 256, 32

    def edit(k, f):
        g = {n: v for n, v in ref.items()}
        g[k] = ref[k].copy()
        f(g[k])
        return g

    def zero_q(v): v[:H] = 0
    def negate_q(v): v[:H] *= -1
    def double_q(v): v[:H] *= 2

    def swap_k_heads(v):
        a, b = H + 2 * dh, H + 5 * dh
        t = v[a:a + dh].copy(); v[a:a + dh] = v[b:b + dh]; v[b:b + dh] = t
    return [("kg2rg q weight block zeroed", edit(KG2RG_W, zero_q), "kg2rg in_proj_weight q rows"),
            ("kg2rg q weight block negated", edit(KG2RG_W, negate_q), "kg2rg in_proj_weight q rows"),
            ("kg2rg q weight block doubled", edit(KG2RG_W, double_q), "kg2rg in_proj_weight q rows"),
            ("rg2kg k weight block, heads 2 and 5 exchanged", edit(RG2KG_W, swap_k_heads), "rg2kg in_proj_weight k rows, head 2"),
            ("rg2kg q bias block zeroed", edit(RG2KG_B, zero_q), "rg2kg in_proj_bias q rows")]


@pytest.mark.parametrize("sharp", [False, True], ids=["make_params", "sharp_params"])
def test_tensor_bounds_are_blind_to_a_wrong_block_and_the_block_check_is_not(sharp):
    """``ref`` = raw_grads of the bf16-operand oracle, ``got`` = ``ref`` with ONE block corrupted.  At OP.make_params every one of
    the five corruptions passes the acceptance of the bf16 training tests and fails the block check at its cap, 0.25.
    At sharp parameters the blocks weigh ten times more in their tensors (kg2rg q: 9.4e-3; rg2kg q / k and q bias: 2.2e-2 / 2.5e-2 /
    2.2e-2 of the tensor), so only the corruptions that move the tensor by less than its 1e-2 stay hidden there -- the zeroed and the
    doubled kg2rg q block, at 0.94 of the bound; the negated block (1.9e-2), the exchanged heads (1.8e-2) and the zeroed bias
    (2.2e-2) are seen by the per-tensor bound at that gain, which is printed, not asserted.  The block check sees all five in both."""
    ref = _oracle_step(sharp, True)
    for what, got, label in _corruptions(ref):
        total, per = _tensor_acceptance(got, ref)
        hidden = total < 2e-3 and per[0][0] < 1e-2
        print(f"{what}: per-tensor acceptance {'passes' if hidden else 'FAILS'}: global {total:.2e}, worst tensor {per[0][0]:.2e} {per[0][1]}")
        if not sharp or what.endswith(("q weight block zeroed", "q weight block doubled")):
            assert hidden, (what, total, per[:2])
        with pytest.raises(AssertionError, match=label) as ex:
            assert_attention_grad_blocks_close(got, ref, ATTN_BLOCK_CAP, what)
        print("   block check:", str(ex.value)[:200])
    assert_attention_grad_blocks_close(ref, ref, ATTN_BLOCK_CAP, "got = ref")
    rs = np.random.RandomState(0)
    noisy = {k: (v * (1.0 + 0.01 * rs.standard_normal(v.shape))).astype(np.float32) for k, v in ref.items()}
    w, h = assert_attention_grad_blocks_close(noisy, ref, ATTN_BLOCK_CAP, "1 % relative Gaussian noise")
    assert 5e-3 < w < 2e-2 and 1e-3 < h < 2e-2, (w, h)


def test_attention_grad_blocks_follow_the_config():
    """The cuts follow hidden_dim and num_heads: 10 whole blocks and 4 x num_heads head blocks, for the default dims and for
    small_a's (H 64, 4 heads of 16 rows); the bias' k rows are not among them."""
    for over, H, nh in (({}, 256, 8), (dict(rg_dim=32, kg_dim=48, hidden_dim=64, num_heads=4), 64, 4)):
        cfg = OP.full_cfg(over)
        g = {k: np.arange(v.size, dtype=np.float32).reshape(v.shape) for k, v in OP.make_params(cfg, 0).items()}
        blocks = list(attention_grad_blocks(g, cfg))
        assert len(blocks) == 10 + 4 * nh and len({l for l, _ in blocks}) == len(blocks)
        assert sorted(a.shape for l, a in blocks if "head" not in l) == sorted([(H, H)] * 6 + [(H,)] * 4)
        assert all(a.shape == (H // nh, H) for l, a in blocks if "head" in l)
        d = dict(blocks)
        assert d["kg2rg in_proj_weight k rows, head 1"][0, 0] == (H + H // nh) * H and d["rg2kg in_proj_bias v rows"][0] == 2 * H
        assert not any("bias k" in l for l, _ in blocks)


# ------------------------------------------------------------------------------------------------------------------------ GPU
ROW, WIDE1, WIDE2P, PSP = {}, dict(wide2=1, wide2_bwd=1), dict(wide2=1, wide2_bwd=1, param_space=1), dict(param_space=1)
GPU_CASES = [                                                       # (nrs, Nk, options, parameter seed)
    ([1], 13, ROW, PSEED),                                          # row-space backward, form by size
    ([33, 32, 64], 16, ROW, PSEED),
    ([33, 32, 64], 1, ROW, PSEED),                                  # (every map is one column)
    (HEADLINE_PLAN, 13, ROW, PSEED),                                # the headline plan: one-launch tail
    (B17, 13, ROW, PSEED),
    ([33, 32, 64], 16, dict(exp=32), PSEED),                        # the KG rows' dQ2 chain finished by bwd2's last-arriving block ...
    ([33, 32, 64], 16, dict(exp=64), PSEED),                        # ... and by the weight-gradient launch (GF_KGQ)
    (HEADLINE_PLAN, 13, dict(exp=32), PSEED),
    (HEADLINE_PLAN, 13, dict(exp=64), PSEED),
    (NRS6, 13, WIDE1, PSEED),                                       # 64-row forward, bwd1w_kernel
    (NRS6, 13, WIDE2P, PSEED),                                      # ... + bwd2w_kernel + bwd2w_finish_kernel
    ([64] * 17, 13, WIDE2P, PSEED),
    ([5, 700, 32], 16, PSP, PSEED),                                 # bwd2p_kernel + unfold_kernel on the 32-row kernels
]
GPU_IDS = [f"nrs{len(n)}x{n[0]}-nk{k}-" + ("_".join(f"{a}{b}" for a, b in o.items()) or "by_size") for n, k, o, _ in GPU_CASES]
# Outputs and loss terms at gain 12 stay at the bounds of test_hip_fused.py::_training_step_shape_envelope: measured over GPU_CASES on
# an MI355X, max |output error| 6.6e-6 against the bf16-operand oracle and 3.9e-4 against the f32 oracle, loss terms 4.5e-6
OUT_ATOL_BF16, OUT_ATOL_F32, TERMS_ATOL, TERMS_RTOL = 5e-4, 1e-3, 2e-3, 1e-3


def _opt(name, value):
    from camouflage_multimodal_amd import _lib
    _lib.check(_lib.lib().camo_debug_set_option(name.encode(), value), "camo_debug_set_option")


@pytest.fixture
def sched_opts():
    yield _opt
    _opt("exp", 0); _opt("wide2", -1); _opt("wide2_bwd", -1); _opt("param_space", -1)


def _case_oracle(cfg, nrs, opts, pseed):
    return bf16_oracle(cfg, _sharp_params(cfg, pseed), nrs, bool(opts.get("wide2")))


def _assert_maps_are_sharp(cfg, nrs, nk, pseed):
    """On the f32 oracle's eval maps, before any kernel is looked at.  A map with one column has no spread: RG->KG at Nk = 1,
    KG->RG of a one-node sample."""
    rgl, kg = _inputs(tuple(nrs), nk)[:2]
    ev, _ = FO.FusionOracle(cfg, _sharp_params(cfg, pseed)).forward_list(rgl, kg)
    long = [b for b in range(len(nrs)) if nrs[b] > 1]
    spread = {}
    if nk > 1:
        spread["rg2kg"] = _log_spread([ev["attn_rg2kg"][b] for b in range(len(nrs))])
        if long:
            spread["kg2rg"] = _log_spread([ev["attn_kg2rg"][b] for b in long])
    assert all(v > 0.5 for v in spread.values()), f"attention maps too close to uniform: log-P spread {spread}"
    return spread


@pytest.mark.parametrize("nrs,nk,opts,pseed", GPU_CASES, ids=GPU_IDS)
def test_sharp_cases_have_sharp_maps_and_few_units_at_the_relu_threshold(nrs, nk, opts, pseed):
    """What the GPU cases rest on, checked without a GPU: the maps' log-P spread > 0.5 in both directions, and the first pass of
    the bf16-operand oracle finds at most oracle_step_at_relu_thresholds' default budget of 6 tail units within 5e-5 of the ReLU
    threshold (a case over the budget gets another parameter seed, never a wider budget)."""
    cfg = OP.full_cfg()
    spread = _assert_maps_are_sharp(cfg, nrs, nk, pseed)
    rgl, kg, y, e, s = _inputs(tuple(nrs), nk)
    orc = _case_oracle(cfg, nrs, opts, pseed)
    orc.near, orc.near_eps = [], 5e-5
    FO.train_step(orc, FO.AdamW(orc.p), rgl, kg, y, e, s, training=True, seed=DSEED)
    print(f"log-P spread {spread}; tail units within 5e-5 of the ReLU threshold: {len(orc.near)}")
    assert len(orc.near) <= 6, orc.near


@pytest.mark.gpu
@pytest.mark.parametrize("nrs,nk,opts,pseed", GPU_CASES, ids=GPU_IDS)
def test_bf16_training_step_at_sharp_parameters_block_by_block(nrs, nk, opts, pseed, sched_opts):
    """One train_raw step (bf16, dropout 0.3, q / k rows x 12) on the form of the backward that ``opts`` selects, against FO.train_step
    of the bf16-operand oracle after the ReLU decisions at the threshold are settled: outputs, loss terms and the two tensor-level
    bounds as in test_hip_fused.py::_training_step_shape_envelope, then the attention gradients block by block and head by head.
    Shapes are the smallest that reach each path: one row, partial / exact / double tiles, Nk = 1 and 16, the headline plan's
    one-launch tail, B = 17, two samples in one 64-row block."""
    import torch
    from test_hip_parity import make_model, outs6, t2n
    cfg = OP.full_cfg()
    _assert_maps_are_sharp(cfg, nrs, nk, pseed)
    for name, value in opts.items():
        sched_opts(name, value)
    m = make_model(cfg, pseed, "bf16", params=_sharp_params(cfg, pseed)).train()
    eng = m._engine
    rgl, kg, y, e, s = _inputs(tuple(nrs), nk)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    outs, terms, _ = eng.train_raw(batch, eng.workspace(batch, private=True), torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s),
                                   True, DSEED, eng._gtab)
    torch.cuda.synchronize()
    outs, terms = t2n(outs), t2n(terms)
    grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    assert np.isfinite(outs).all() and all(np.isfinite(v).all() for v in grads.values())
    ref32, _ = FO.FusionOracle(cfg, _sharp_params(cfg, pseed)).forward_list(rgl, kg, training=True, seed=DSEED)
    ref, near, flipped = oracle_step_at_relu_thresholds(
        lambda: _case_oracle(cfg, nrs, opts, pseed),
        lambda o: FO.train_step(o, FO.AdamW(o.p), rgl, kg, y, e, s, training=True, seed=DSEED), grads)
    if near:
        print("tail units at the ReLU threshold (site, sample, unit, pre-activation):", near, "taken flipped:", flipped)
    total, per = _tensor_acceptance(grads, ref["raw_grads"])
    t_err = np.abs(terms - ref["loss_terms"])
    print(f"sharp parameters, nrs={nrs[:6]} nk={nk} {opts}: max |output err| vs the bf16-operand oracle {np.abs(outs - outs6(ref['outs'])).max():.2e}, "
          f"vs the f32 oracle {np.abs(outs - outs6(ref32)).max():.2e}; loss terms: max |err| {t_err.max():.2e}, max err / (atol + rtol |want|) "
          f"{(t_err / (TERMS_ATOL + TERMS_RTOL * np.abs(ref['loss_terms']))).max():.3f}; global relative gradient error {total:.5f}; "
          f"worst {per[0][1]} {per[0][0]:.4f}")
    failures = []
    for check in (lambda: assert_close(outs, outs6(ref32), OUT_ATOL_F32, 0, "outputs vs the f32 oracle"),
                  lambda: assert_close(outs, outs6(ref["outs"]), OUT_ATOL_BF16, 0, "outputs vs the bf16-operand oracle"),
                  lambda: assert_close(terms, ref["loss_terms"], TERMS_ATOL, TERMS_RTOL, "loss terms"),
                  lambda: assert_attention_grad_blocks_close(grads, ref["raw_grads"], ATTN_BLOCK_BOUND, f"nrs={nrs[:6]} nk={nk} {opts}",
                                                                     single_column=single_column_attentions(nrs, nk))):
        try:                                                                   # (report every figure that is off, not just the first)
            check()
        except AssertionError as ex:
            failures.append(str(ex)[:600])
    assert not failures, "\n".join(failures)
    assert total < 2e-3, (total, per[:4])
    assert per[0][0] < 1e-2, per[:4]
