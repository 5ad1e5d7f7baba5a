"""Each size-selected kernel on both sides of its switch point, reached by SIZE alone (no option is touched).  Needs an MI355X.

The schedule of a call follows from its arguments: the longest sample (max_nr), the packed rows T, the sample count B and Nk.
The other test files run the kernels at the sizes they were built for; here every case sits on one side of a limit, usually with
one long sample that moves the short ones (some of one row) onto the long sample's kernel, where most of their tiles are empty.

A. Exact f32 (the default precision), default dims (H 256, 8 heads: head_dim 32), dropout 0.3.  For head_dim 32 and Nk <= 16,
   launch_attn_kg2rg_{fwd,bwd} (csrc/attn.hip) choose by max_nr alone:
     max_nr <= 768 = 8 waves x 6 tiles x 16 keys (attn_mfma_ok)          kg2rg_fwd_mfma_kernel / kg2rg_bwd_mfma_kernel
     769 ... 1038                                                        kg2rg_fwd32_kernel    / kg2rg_bwd32_kernel
     1039 ... 2108                                                       kg2rg_fwd32_kernel    / attn_kg2rg_bwd_kernel<16>
     >= 2109                                                             attn_kg2rg_fwd_kernel<16> / attn_kg2rg_bwd_kernel<16>
   (csrc/attn_fast.hip, kg2rg32_lds() <= FAST_LDS_BUDGET = 150 KiB = 38 400 floats with NKP = 16, DH = 32: the backward needs
   2*16*32 + 4*16 + 8*16*32 + 2*16*m = 5184 + 32 m floats -> m <= 1038, the forward 4672 + 16 m -> m <= 2108.)
   Nk > 16 takes the <64> instantiations of all four general attention kernels.  Each case: one NativeTrainer step against the
   oracle's train step with the same seed (the kernels regenerate its counter-hash dropout masks), and an eval forward with
   attention maps against the oracle.
B. The bf16 product schedule (csrc/fusion_abi.hip) past the Nr <= 530 of the real histogram: the wide front half's and the 64-row
   forward's max_nr limits, the fused schedule's own limit (64 x FUSED_MAX_SPLITS = 4096 rows) -- against the bf16-operand oracle.
"""
import numpy as np
import pytest
import torch

from helpers import QK_GAIN, _log_spread, _sharp_params, assert_close, oracle_batch_step
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_hip_large_batch import _histogram_batch, _packed_forward, _train_step_vs_bf16_oracle
from test_hip_parity import make_model, outs6, t2n

pytestmark = pytest.mark.gpu

DSEED = 0x0123456789ABCDEF
SMALL_A = dict(rg_dim=32, kg_dim=48, hidden_dim=64, num_heads=4)       # (tests/golden train_small_a: head_dim 16)


def _f32_case(cfg, pseed, nrs, nk, y=None):
    """One f32 training step (dropout as in ``cfg``) through NativeTrainer against FO.train_step with the same seed, at the bounds of
    test_train_mode_dropout_matches_oracle_masks; before it, an eval forward with attention maps against the oracle's: logits and
    both maps at the bounds of test_long_sequence_config_nr2048 / test_eval_forward_golden_real_kg, every map row summing to 1.
    Parameters from _sharp_params, so that the attention maps are far from uniform (checked on the oracle's maps).
    ``y``: mask labels instead of OP.make_labels' (which are 0 / 1 whatever num_classes is)."""
    from camouflage_multimodal_amd import NativeTrainer
    B = len(nrs)
    rg = [OP.make_rg(n, cfg["rg_dim"], seed=700 + 3 * pseed + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, cfg["kg_dim"], seed=800 + 3 * pseed + i) for i in range(B)])
    y0, e, s = OP.make_labels(B, seed=40 + pseed)
    y = y0 if y is None else np.asarray(y, np.int64)
    rgp, kgt = torch.from_numpy(np.concatenate(rg)).cuda(), torch.from_numpy(kg).cuda()
    prm = _sharp_params(cfg, pseed)
    m = make_model(cfg, pseed, params=prm).eval()
    orc = FO.FusionOracle(cfg, {k: v.copy() for k, v in prm.items()})
    ref_eval, _ = orc.forward_list(rg, kg)
    long = [b for b in range(B) if nrs[b] > 1]
    spread = (_log_spread([ref_eval["attn_rg2kg"][b] for b in long]), _log_spread([ref_eval["attn_kg2rg"][b] for b in long]))
    assert min(spread) > 0.5, f"attention maps too close to uniform to show an error in the scores: log-P spread {spread}"
    with torch.no_grad():
        o = m.forward_packed(rgp, list(nrs), kgt, return_attention=True)
    assert_close(np.concatenate([t2n(v) for v in o[:4]], axis=1), outs6(ref_eval), 2e-5, 1e-5, f"eval logits nrs={nrs} nk={nk}")
    for b in range(B):
        assert_close(t2n(o[4]["rg2kg"][b]), ref_eval["attn_rg2kg"][b], 2e-6, 1e-4, f"attn rg2kg sample {b} (Nr {nrs[b]})")
        assert_close(t2n(o[4]["kg2rg"][b]), ref_eval["attn_kg2rg"][b], 2e-7, 2e-4, f"attn kg2rg sample {b} (Nr {nrs[b]})")
        assert_close(t2n(o[4]["rg2kg"][b]).sum(1), np.ones(nrs[b]), 1e-5, 0, "rg2kg rows sum to 1")
        assert_close(t2n(o[4]["kg2rg"][b]).sum(1), np.ones(nk), 1e-5, 0, "kg2rg rows sum to 1")
    m.train()
    tr = NativeTrainer(m, keep_grads=True)
    ref = FO.train_step(orc, FO.AdamW(orc.p), rg, kg, y, e, s, training=True, seed=DSEED)
    terms, _ = tr.step(rgp, list(nrs), kgt, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), seed=DSEED)
    assert_close(t2n(terms), ref["loss_terms"], 3e-5, 2e-4, f"loss terms nrs={nrs} nk={nk}")
    coef = min(1.0, 1.0 / (float(ref["grad_norm"]) + 1e-6))
    tr.engine.ensure_flat_grads(attach=True)
    for k, p in m.named_parameters():
        want = ref["raw_grads"][k]
        rms = float(np.sqrt((want.astype(np.float64) ** 2).mean()))
        assert_close(t2n(p.grad) / coef, want, 5e-4 * rms + 2e-7, 5e-4, f"grad {k} nrs={nrs} nk={nk}")


# (max_nr, batch): the long sample first in some, last in others; one-row samples in every batch
KG2RG_CASES = [
    (768, [768, 1, 45, 1, 300]),
    (769, [1, 300, 45, 1, 769]),
    (1038, [1038, 1, 200, 7]),
    (1039, [5, 1, 130, 1039]),
    (2108, [2108, 1, 64, 1]),
    (2109, [1, 33, 1, 2109]),
]


@pytest.mark.parametrize("max_nr,nrs", KG2RG_CASES, ids=[f"max_nr{m}" for m, _ in KG2RG_CASES])
def test_f32_kg2rg_attention_switch_by_max_nr(max_nr, nrs):
    """f32 training + eval at Nk = 13 with max_nr on each side of the three KG->RG switch points (module docstring A):
    768 -> kg2rg_fwd_mfma_kernel / kg2rg_bwd_mfma_kernel (the last max_nr with 8 waves x 6 tiles x 16 keys);
    769 and 1038 -> kg2rg_fwd32_kernel / kg2rg_bwd32_kernel (1038: 5184 + 32 * 1038 = 38 400 floats, the backward's LDS budget);
    1039 and 2108 -> kg2rg_fwd32_kernel / attn_kg2rg_bwd_kernel<16> (2108: 4672 + 16 * 2108 = 38 400, the forward's budget);
    2109 -> attn_kg2rg_fwd_kernel<16> / attn_kg2rg_bwd_kernel<16>.  The short samples run on the long sample's kernel."""
    assert max(nrs) == max_nr
    _f32_case(OP.full_cfg(dict(dropout=0.3)), 20 + max_nr % 7, nrs, 13)


@pytest.mark.parametrize("nk", [16, 17, 64])
def test_f32_training_nk_switch_default_dims(nk):
    """Nk <= 16 runs the MFMA attention kernels (attn_mfma_ok: Nk <= 16); Nk = 17 and 64 the general ones in their <64>
    instantiations (DISPATCH_NK: Nk > 16), both directions, forward and backward, at head_dim 32 -- with dropout 0.3."""
    _f32_case(OP.full_cfg(dict(dropout=0.3)), 30 + nk, [530, 1, 64, 303], nk)


def test_f32_training_nk17_head_dim16():
    """Nk = 17 where head_dim is 16 (small_a's dims: H 64, 4 heads): no MFMA or fast attention kernel takes it (both need
    head_dim 32), so the general <64> kernels run with another G = 256 / dh grouping of the KG->RG heads."""
    _f32_case(OP.full_cfg(dict(SMALL_A, dropout=0.3)), 3, [40, 1, 130], 17)


def test_nk65_is_refused_and_computes_nothing():
    """Nk = 65 is past the general attention kernels' one-key-per-lane KG side (attn_supported: Nk <= 64): the library refuses the
    call with CAMO_E_UNSUPPORTED before it launches anything -- the outputs it was handed stay as they were -- and the Python surface
    raises CamoError without touching parameters or gradients."""
    import ctypes as C
    from camouflage_multimodal_amd import NativeTrainer, _lib
    cfg = OP.full_cfg(dict(dropout=0.3))
    m = make_model(cfg, 2).train()
    nrs = [40, 1]
    rgp = torch.from_numpy(np.concatenate([OP.make_rg(n, 128, seed=i) for i, n in enumerate(nrs)])).cuda()
    kg65 = torch.from_numpy(np.stack([OP.make_kg(65, 128, seed=60 + i) for i in range(2)])).cuda()
    eng = m._engine
    L = _lib.lib()
    assert L.camo_workspace_bytes(C.byref(eng.dims), 2, 41, 64) > 0
    assert L.camo_workspace_bytes(C.byref(eng.dims), 2, 41, 65) == 0
    assert b"Nk <= 64" in L.camo_last_error()
    # the raw call, with a workspace large enough for Nk = 64 and sentinel-filled outputs
    batch = eng.make_batch(rgp, nrs, kg65[:, :64].contiguous())
    ws = eng.workspace(batch, private=True)
    outs = torch.full((2, eng.out_width), float("nan"), device="cuda")
    a1 = torch.full((41, 65), -7.0, device="cuda"); a2 = torch.full((41, 65), -7.0, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = L.camo_forward(C.byref(eng.dims), eng._ptab, P(rgp), P(batch.offsets), P(batch.desc), P(kg65), 2, 41, 65, 40,
                        P(ws), ws.numel(), P(outs), P(a1), P(a2), 1, DSEED, 0, 0, None)
    torch.cuda.synchronize()
    assert rc == -2, (rc, L.camo_last_error())                                   # CAMO_E_UNSUPPORTED
    assert torch.isnan(outs).all() and (a1 == -7.0).all() and (a2 == -7.0).all()
    # the public surface: eval forward and a training step both refuse, parameters and gradients untouched
    before = {k: t2n(v).copy() for k, v in m.state_dict().items()}
    tr = NativeTrainer(m, keep_grads=True)
    eng.ensure_flat_grads(attach=True).fill_(3.0)
    y, e, s = OP.make_labels(2, seed=1)
    with pytest.raises(_lib.CamoError, match="Nk <= 64"):
        tr.step(rgp, nrs, kg65, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), seed=DSEED)
    with pytest.raises(_lib.CamoError, match="Nk <= 64"):
        with torch.no_grad():
            m.eval().forward_packed(rgp, nrs, kg65)
    torch.cuda.synchronize()
    assert all(np.array_equal(t2n(v), before[k]) for k, v in m.state_dict().items())
    assert (eng.ensure_flat_grads(attach=True) == 3.0).all()


def test_f32_training_large_t_histogram_b128(kg_real):
    """B = 128 samples of the real Nr histogram (~60 k packed rows), f32, dropout 0.3: the weight gradients of the node-level
    layers run through gemm.hip's split-K over tens of thousands of rows with fp32 atomics.  The raw (unclipped) gradients of one
    training call against the oracle's, summed one sample at a time, at the bounds of the f32 dropout cases.  At this size a few
    first-FFN-layer pre-activations sit within the kernels' f32 rounding of zero (measured: 2 of 31 M, ~2e-7 away); the oracle takes
    those decisions as the kernels did (_f32_batch_reference)."""
    cfg = OP.full_cfg(dict(dropout=0.3))
    B, pseed = 128, 7
    nrs, rg, kg = _histogram_batch(B, 30, kg_real)
    assert sum(nrs) >= 57344, sum(nrs)
    m = make_model(cfg, pseed).train()
    eng = m._engine
    y, e, s = OP.make_labels(B, seed=22)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    ws = eng.workspace(batch, private=True)
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    outs, terms, _ = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, DSEED, eng._gtab)
    torch.cuda.synchronize()
    grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    ref = _f32_batch_reference(cfg, pseed, rg, kg, y, e, s, grads)
    print(f"f32 B = {B} (T = {sum(nrs)}): ReLU decisions at the threshold taken flipped: {ref['flips']}")
    assert_close(t2n(outs), outs6(ref["outs"]), 2e-5, 1e-5, "outputs")
    assert_close(t2n(terms), ref["loss_terms"], 3e-5, 2e-4, "loss terms")
    for k in grads:
        want = ref["raw_grads"][k]
        assert_close(grads[k], want, _f32_grad_atol(want), 5e-4, f"grad {k} at T = {sum(nrs)}")


def _f32_grad_atol(want):
    return 5e-4 * float(np.sqrt((want.astype(np.float64) ** 2).mean())) + 2e-7


def _f32_batch_reference(cfg, pseed, rg, kg, y, e, s, grads):
    """The oracle's raw gradients of the batch with its ReLU decisions at the threshold settled as the kernels took them: the tail
    units within 1e-5 (f32 pre-activations agree to ~1e-6 there), then, for the first FFN layers' units whose gradient rows are
    still off, their node-level decisions within 1e-6 of zero (helpers.oracle_batch_step; one pass over the batch)."""
    def node_off(g):
        off = {}
        for site, k in ((FO.SITE_FFN_RG, "fusion.ffn_rg.0.weight"), (FO.SITE_FFN_KG, "fusion.ffn_kg.0.weight")):
            want = g[k].astype(np.float64)
            bad = np.abs(grads[k] - want) > _f32_grad_atol(want) + 5e-4 * np.abs(want)
            if bad.any():
                off[site] = sorted(set(int(u) for u in np.nonzero(bad)[0]))
        if off:
            print("first-FFN-layer gradient rows off before the node-level ReLU treatment:", off)
        return off
    return oracle_batch_step(lambda: FO.FusionOracle(cfg, OP.make_params(cfg, pseed)), rg, kg, y, e, s, DSEED, grads, near_eps=1e-5,
                             node_off=node_off)


# ---------------------------------------------------------------------------------------------------------------------- B. bf16
def _long_plus(n_long, n_short, at, base=440):
    nrs = [base + 3 * (i % 7) for i in range(n_short)]
    nrs.insert(at, n_long)
    return nrs


@pytest.mark.parametrize("max_nr", [2944, 2945])
def test_bf16_training_wide_front_max_nr_limit(max_nr, kg_real):
    """Training at 16 384 <= T < 28 672 (31 samples: one long, 30 of ~450 rows): the front half runs on 64-row blocks
    (make_plan's wide front: 2 sub-tiles from 10 240 rows) while max_nr <= wide_max_rows(2) - 64 * 2 = 32 * 2 * 48 - 128 = 2944;
    at 2945 it falls back to the 32-row front_kernel.  From 16 384 rows the first backward half is bwd1w_kernel / bwd2w_kernel on
    64-row half-blocks, where the long sample spans ~46 of them."""
    nrs = _long_plus(max_nr, 30, 0 if max_nr == 2944 else 30)
    assert 16384 <= sum(nrs) < 28672 and max(nrs) == max_nr
    _train_step_vs_bf16_oracle(len(nrs), 8, kg_real, nrs=nrs)


def test_bf16_training_128row_front_4096_row_sample(kg_real):
    """Training at 28 672 <= T < 57 344 with B = 60 and one 4 096-row sample (the fused schedule's limit, 64 x FUSED_MAX_SPLITS):
    the 128-row front (make_plan's wide front: 4 sub-tiles from 4 x 32 x 224 rows; 4096 <= wide_max_rows(4) - 256) and, at
    49 <= B <= 64 with no wide forward to build the two-plane tail's weight planes, the nine-launch tail."""
    nrs = _long_plus(4096, 59, 17)
    assert 28672 <= sum(nrs) < 57344 and 49 <= len(nrs) <= 64
    _train_step_vs_bf16_oracle(len(nrs), 9, kg_real, nrs=nrs)


def test_bf16_training_64row_forward_4096_row_sample(kg_real):
    """Training at T >= 57 344 (120 samples of the real histogram + one of 4 096 rows): the saving + dropout variants of
    rgfwd2_kernel / kgchain_kernel (make_plan: max_nr <= wide2_max_rows() = 4096) with the long sample across 64 half-blocks,
    the two-plane tail, bwd1w_kernel / bwd2w_kernel -- against the oracle with the 64-row forward's flash-block partition."""
    nrs, _, _ = _histogram_batch(120, 17, kg_real)
    nrs.insert(61, 4096)
    assert sum(nrs) >= 57344, sum(nrs)
    _train_step_vs_bf16_oracle(len(nrs), 6, kg_real, nrs=nrs)


@pytest.mark.parametrize("max_nr", [4096, 4097])
def test_bf16_inference_fused_schedule_max_nr_limit(max_nr, kg_real):
    """Eval forward at T >= 10 240: with max_nr = 4096 the fused schedule's 64-row inference forward (rgfwd2_kernel, CAMO_BACK_RG_64);
    at 4097 both make_plan's fused rule (max_nr <= 64 x FUSED_MAX_SPLITS) and its bf16 rule (the MFMA KG->RG kernels' max_nr <= 768) refuse the
    call, which then runs the general bf16-operand path, KG->RG attention on the general forward attn_kg2rg_fwd_kernel<16>.
    Logits of the long sample, its neighbours and the first and last samples against the f32 oracle at north_star's 1e-3, and
    packed == one-by-one at the bound of the B = 256 case."""
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    nrs, rg, kg = _histogram_batch(16, 18, kg_real)
    at = 8
    nrs.insert(at, max_nr)
    rg.insert(at, OP.make_rg(max_nr, 128, seed=4321))
    kg = np.concatenate([kg[:at], kg_real[None] * np.float32(0.97), kg[at:]]).astype(np.float32)
    assert sum(nrs) >= 10240 and max(nrs) == max_nr
    got = _packed_forward(m, rg, nrs, kg)
    assert np.isfinite(got).all()
    picks = [0, at - 1, at, at + 1, len(nrs) - 1]
    ref, _ = FO.FusionOracle(cfg, OP.make_params(cfg, 0)).forward_list([rg[b] for b in picks], kg[picks])
    assert_close(got[picks], outs6(ref), 1e-3, 0, f"max_nr {max_nr} packed forward vs the f32 oracle")
    singles = np.stack([_packed_forward(m, [rg[b]], [nrs[b]], kg[b:b + 1])[0] for b in picks])
    assert_close(got[picks], singles, 4e-4, 0, "packed == one-by-one")
