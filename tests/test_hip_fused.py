"""The fused row-tile schedule (csrc/fused_rows.hip) against the oracle, stage by stage.  Needs an MI355X.

The kernels keep a 32-row tile on chip through a chain of layers, so a wrong fragment map anywhere shows up only in the
logits unless the intermediates are looked at: the testing hook ``fused_save`` makes an inference call write every tensor
a backward would read, and each is compared with the oracle's cache at bf16 tolerances."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_attention_grad_blocks_close, assert_close, bf16_oracle, oracle_step_at_relu_thresholds, single_column_attentions
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_fragment_maps import frag_order
from test_hip_parity import make_model, outs6, t2n

pytestmark = pytest.mark.gpu


def _opt(name, value):
    from camouflage_multimodal_amd import _lib
    _lib.check(_lib.lib().camo_debug_set_option(name.encode(), value), "camo_debug_set_option")


@pytest.fixture
def fused_opts():
    yield _opt
    _opt("fused", -1); _opt("fused_save", 0); _opt("sched16", -1); _opt("tail17", -1); _opt("fused_rt", -1); _opt("tailw", -1); _opt("fused_one", 1); _opt("tn_big", -1); _opt("param_space", -1); _opt("tailw_bwd", -1); _opt("wide2", -1); _opt("wide2_bwd", -1)


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (u.astype(np.uint32) << 16).view(np.float32)


def _ws_raw(eng, batch, ws, name, nbytes):
    from camouflage_multimodal_amd import _lib
    off = _lib.lib().camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
    assert off >= 0, name
    return ws[off:off + nbytes].cpu().numpy().copy()


def ws_bf16(eng, batch, ws, name, rows, cols):
    raw = _ws_raw(eng, batch, ws, name, 2 * rows * cols).view(np.uint16).astype(np.uint32)
    return (raw << 16).view(np.float32).reshape(rows, cols)


def ws_f32(eng, batch, ws, name, n):
    return _ws_raw(eng, batch, ws, name, 4 * n).view(np.float32)


def close_rel(got, want, rel, what, mean_rel=None, flips=0.0):
    """max |err| <= rel * max|want| (and mean |err| <= mean_rel * max|want|).  ``flips``: fraction of elements allowed outside
    the max bound -- gradients downstream of a ReLU unit whose bf16 pre-activation sits within rounding of 0 flip between
    their full value and 0, which says nothing about the kernel; the mean bound still holds them to account."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    scale = max(float(np.abs(want).max()), 1e-6)
    err = np.abs(got - want)
    bad = float((err > rel * scale).mean())
    assert bad <= flips, (f"{what}: {bad:.5f} of the elements outside {rel} * scale {scale:.3e}; max |err| {err.max():.3e} at "
                          f"{np.unravel_index(err.argmax(), err.shape)}")
    if mean_rel is not None:
        assert err.mean() <= mean_rel * scale, f"{what}: mean |err| {err.mean():.3e} (scale {scale:.3e})"


NRS = [303, 64, 1, 530, 65, 127, 31, 32, 33]


@pytest.mark.parametrize("rt", [0, 1, 2, 4, 64])
@pytest.mark.parametrize("training", [False, True])
def test_fused_forward_stage_by_stage(training, rt, kg_real, fused_opts):
    """rt = 0: the 32-row tile kernels (fused_rows.hip); rt = 1, 2, 4: the wide-tile kernels (fused_wide.hip) with that many
    32-row tiles per block; rt = 64: the 64-row half-blocks of 4 waves + the KG rows' launch (fused_wide2.hip, saving / dropout
    variants) -- the same saved tensors, pooled sums and logits."""
    if rt == 64:
        fused_opts("wide2", 1)
    else:
        fused_opts("fused_rt", rt); fused_opts("wide2", 0)
    cfg = OP.full_cfg()
    prm = OP.make_params(cfg, 0)
    m = make_model(cfg, 0, "bf16")
    m.train(training)
    eng = m._engine
    B, T, Nk = len(NRS), sum(NRS), 13
    rg = [OP.make_rg(n, 128, seed=70 + i) for i, n in enumerate(NRS)]
    kg = np.stack([kg_real * (1.0 + 0.05 * i) for i in range(B)]).astype(np.float32)      # (different keys per sample)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), NRS, torch.from_numpy(kg).cuda())
    seed = 0xABCDEF0123
    fused_opts("fused_save", 1)
    ws = eng.workspace(batch, private=True)
    ws.zero_()
    outs, _ = eng.forward_raw(batch, ws, training, seed, inference=True, cache_shadows=False)
    torch.cuda.synchronize()
    orc = FO.FusionOracle(cfg, prm)
    ref, caches = orc.forward_list(rg, kg, training=training, seed=seed)
    cat = lambda k: np.concatenate([c[k] for c in caches])
    H = 256
    sc = np.float32(1.0 / np.sqrt(32.0))
    # weight shadow of the RG in-projections = fragment order of [Wq1; Wk2; Wv2], bf16-rounded, bit for bit
    Wcat = np.concatenate([prm["fusion.cross_attn_rg2kg.in_proj_weight"][:H], prm["fusion.cross_attn_kg2rg.in_proj_weight"][H:]])
    got_sh = ws_bf16(eng, batch, ws, "Wqkv_rg", 1, 768 * 256)[0]
    assert np.array_equal(got_sh, frag_order(bf16_round(Wcat))), "weight shadow order"
    assert np.array_equal(ws_bf16(eng, batch, ws, "W1s", 1, 512 * 256)[0], frag_order(bf16_round(prm["fusion.ffn_rg.0.weight"])))
    # front half
    assert np.array_equal(ws_bf16(eng, batch, ws, "X16", T, 128), bf16_round(np.concatenate(rg)))
    close_rel(ws_bf16(eng, batch, ws, "R16", T, H), cat("R"), 8e-3, "R16")
    close_rel(ws_bf16(eng, batch, ws, "G16", B * Nk, H), cat("G"), 8e-3, "G16")
    close_rel(ws_bf16(eng, batch, ws, "Q16", T, H), cat("Q") * sc, 1.2e-2, "Q16 (pre-scaled)")
    close_rel(ws_bf16(eng, batch, ws, "KV2_16", T, 2 * H), np.concatenate([cat("K2"), cat("V2")], axis=1), 1.2e-2, "KV2_16")
    close_rel(ws_bf16(eng, batch, ws, "Q2_16", B * Nk, H), cat("Q2") * sc, 1.2e-2, "Q2_16 (pre-scaled)")
    close_rel(ws_bf16(eng, batch, ws, "KV16", B * Nk, 2 * H), np.concatenate([cat("Kk"), cat("Vk")], axis=1), 1.2e-2, "KV16")
    # back half
    close_rel(ws_bf16(eng, batch, ws, "O16", T, H), cat("O"), 2e-2, "O16 (RG->KG attention output)", 2e-3)
    close_rel(ws_bf16(eng, batch, ws, "O2_16", B * Nk, H), cat("O2"), 2e-2, "O2_16 (KG->RG attention output)", 3e-3)
    lse = ws_f32(eng, batch, ws, "lse2", B * 8 * 16 * 2).reshape(B, 8, 16, 2)
    for b, c in enumerate(caches):
        S2 = np.einsum("jhd,thd->thj", c["Q2"].reshape(Nk, 8, 32), c["K2"].reshape(-1, 8, 32)) * sc       # [Nr, nh, Nk]
        mx = S2.max(axis=0)
        close_rel(lse[b, :, :Nk, 0], mx, 2e-2, "KG->RG softmax max")
        assert np.allclose(lse[b, :, :Nk, 1], np.exp(S2 - mx).sum(axis=0), rtol=3e-2), "KG->RG softmax sum"
    close_rel(ws_bf16(eng, batch, ws, "XH16", T, H), cat("xh1"), 2.5e-2, "normalised LN input (RG)", 2e-3)
    close_rel(ws_f32(eng, batch, ws, "rstd1", T), cat("rstd1")[:, 0], 1e-2, "rstd (RG)")
    close_rel(ws_bf16(eng, batch, ws, "Y16", T, H), cat("Y"), 2.5e-2, "Y16", 2e-3)
    close_rel(ws_bf16(eng, batch, ws, "Y2_16", B * Nk, H), cat("Y2"), 2.5e-2, "Y2_16", 3e-3)
    close_rel(ws_bf16(eng, batch, ws, "XH2_16", B * Nk, H), cat("xh2"), 2.5e-2, "normalised LN input (KG)", 3e-3)
    close_rel(ws_f32(eng, batch, ws, "Ymean", B * H).reshape(B, H), np.stack([c["Y"].mean(0) for c in caches]), 5e-3, "Ymean")
    close_rel(ws_f32(eng, batch, ws, "Y2mean", B * H).reshape(B, H), np.stack([c["Y2"].mean(0) for c in caches]), 8e-3, "Y2mean")
    close_rel(ws_f32(eng, batch, ws, "H1mean", B * 2 * H).reshape(B, 2 * H), np.stack([c["H1d"].mean(0) for c in caches]), 1e-2, "H1mean")
    close_rel(ws_f32(eng, batch, ws, "H2mean", B * 2 * H).reshape(B, 2 * H), np.stack([c["H2d"].mean(0) for c in caches]), 2e-2, "H2mean")
    # ReLU/dropout bit masks: bit f of row t = (activation after ReLU and dropout > 0); units within bf16 noise of 0 may differ
    for name, key, rows in (("mask1", "H1d", T), ("mask2", "H2d", B * Nk)):
        words = _ws_raw(eng, batch, ws, name, 4 * rows * 16).view(np.uint32).reshape(rows, 16)
        bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(rows, 512).astype(bool)
        want = cat(key) > 0
        near = np.abs(cat(key.replace("d", ""))) < 2e-2                      # pre-dropout activation close to the ReLU threshold
        assert (bits == want)[~near].mean() > 0.9995 and (bits == want).mean() > 0.99, name
    assert_close(t2n(outs), outs6(ref), 1.5e-3 if training else 1e-3, 0, "logits of the fused schedule")
    # and against the bf16-resident schedule of round 1 on the same call
    fused_opts("fused", 0)
    outs16, _ = eng.forward_raw(batch, eng.workspace(batch, private=True), training, seed, inference=True)
    assert_close(t2n(outs), t2n(outs16), 1.5e-3, 0, "fused vs bf16-resident schedule")


@pytest.mark.parametrize("rt", [0, 2, 4])
@pytest.mark.parametrize("nrs,nk", [([1], 1), ([5, 700, 32], 16), ([64] * 40, 13), ([2048, 17], 13), ([128, 256, 127, 129, 1, 383], 13)])
def test_fused_forward_shapes(nrs, nk, rt, fused_opts):
    """Envelope of the fused schedule: one-node samples, Nk = 1 and 16, tiles that end on a sample boundary, more samples than
    KG blocks per wave, a 2048-node sample (64 key chunks per KG block)."""
    fused_opts("fused_rt", rt)
    cfg = OP.full_cfg()
    m = make_model(cfg, 2, "bf16").eval()
    orc = FO.FusionOracle(cfg, OP.make_params(cfg, 2))
    rg = [OP.make_rg(n, 128, seed=7 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, 128, seed=90 + i) for i in range(len(nrs))])
    ref, _ = orc.forward_list(rg, kg)
    with torch.no_grad():
        o = m.forward_packed(torch.from_numpy(np.concatenate(rg)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    got = np.concatenate([t2n(v) for v in o], axis=1)
    assert np.isfinite(got).all()
    assert_close(got, outs6(ref), 1e-3, 0, f"nrs={nrs[:4]} nk={nk}")


@pytest.mark.parametrize("wide2", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("training", [False, True])
def test_fused_backward_stage_by_stage(training, wide2, kg_real, fused_opts):
    """The fused backward kernels against the intermediate activation gradients of the oracle in its bf16-operand mode, then every
    parameter gradient: absolute bounds (global relative error < 0.2 %, every tensor that carries weight < 1 %; measured 0.002-0.01 %
    and <= 0.1 %), no other HIP schedule as a yardstick."""
    fused_opts("wide2", 1 if wide2 in (1, 2, 4) else 0)  # (1: the forward that saves for these backward kernels is the 64-row one, fused_wide2.hip)
    fused_opts("wide2_bwd", 1 if wide2 >= 2 else 0)      # (2: ... and the RG rows' first backward half runs on 64-row half-blocks too, bwd_wide2.hip;
    param_space = wide2 == 4                             #  3: that backward behind the 8-wave forward -- what batches of 16 384 .. 57 343 rows run;
    if param_space:                                      #  4: as 2 with the projections' weight gradients in parameter space, which is what large batches
        fused_opts("param_space", 1)                     #     run: the second half is then bwd2w_kernel + bwd2w_finish_kernel, no dR / dG products)
    wide2 = wide2 in (1, 2, 4)
    cfg = OP.full_cfg()
    prm = OP.make_params(cfg, 0)
    m = make_model(cfg, 0, "bf16")
    m.train(training)
    eng = m._engine
    B, T, Nk, H = len(NRS), sum(NRS), 13, 256
    rg = [OP.make_rg(n, 128, seed=70 + i) for i, n in enumerate(NRS)]
    kg = np.stack([kg_real * (1.0 + 0.05 * i) for i in range(B)]).astype(np.float32)
    y, e, s = OP.make_labels(B, seed=5)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), NRS, torch.from_numpy(kg).cuda())
    seed = 0x1234ABCD5678
    ws = eng.workspace(batch, private=True)
    ws.zero_()
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    orc = bf16_oracle(cfg, OP.make_params(cfg, 0), NRS, wide2)                  # rounds what the kernels round (oracle/fusion_oracle.py)
    ref = FO.train_step(orc, FO.AdamW(orc.p), rg, kg, y, e, s, training=training, seed=seed, debug=True)
    # forward on the HIP path, then backward from the ORACLE's loss gradient: the focal term's gradient is steep in the
    # logits, and this test is about the backward kernels, not about how logit noise moves d(loss)/d(logits)
    outs, _ = eng.forward_raw(batch, ws, training, seed)
    assert_close(t2n(outs), outs6(ref["outs"]), 5e-4, 0, "outputs")
    d_outs = []
    for b in range(B):
        ob = {k: ref["outs"][k][b] for k in ("mask", "instance", "edge", "score")}
        _, _, d = FO.sample_loss(ob, int(y[b]), float(e[b]), float(s[b]))
        d_outs.append(np.concatenate([d["mask"], d["instance"], d["edge"].reshape(-1), d["score"].reshape(-1)]))
    d_outs = torch.from_numpy(np.stack(d_outs).astype(np.float32)).cuda()
    eng.backward_raw(batch, ws, outs, d_outs, training, seed, eng._gtab)
    torch.cuda.synchronize()
    # tail units whose pre-activation is within 5e-5 of the ReLU threshold may land on either side (helpers.py bounds how many): this
    # batch has three, and which side the kernels take moves with the summation order of the pooled means in front of them
    got_grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    ref, near, flipped = oracle_step_at_relu_thresholds(
        lambda: bf16_oracle(cfg, OP.make_params(cfg, 0), NRS, wide2),
        lambda o: FO.train_step(o, FO.AdamW(o.p), rg, kg, y, e, s, training=training, seed=seed, debug=True), got_grads)
    if near:
        print("tail units at the ReLU threshold (site, sample, unit, pre-activation):", near, "taken flipped:", flipped)
    dbg, caches = ref["dbg"], ref["caches"]
    failures = []

    def close_rel(*a, **k):                    # (report every stage that is off, not just the first)
        try:
            globals()["close_rel"](*a, **k)
        except AssertionError as ex:
            failures.append(str(ex)[:300])
    cat = lambda k: np.concatenate([d[k] for d in dbg])
    # stage bounds against the bf16-operand oracle: <= 0.2 % of the elements further than 2 % of the tensor's maximum (a bf16 value
    # that lands on the other side of a rounding boundary moves by 0.4 % of itself; sums of such values by less), mean error <= 0.3 %
    R, M, F = 2e-2, 3e-3, 2e-3
    close_rel(ws_bf16(eng, batch, ws, "dH16", T, 2 * H), cat("dH_ffn_rg"), R, "dH (RG)", M, flips=F)
    close_rel(ws_bf16(eng, batch, ws, "dH2_16", B * Nk, 2 * H), cat("dH_ffn_kg"), R, "dH (KG)", M, flips=F)
    close_rel(ws_bf16(eng, batch, ws, "dU16", T, H), cat("dU"), R, "dU", M, flips=F)
    close_rel(ws_bf16(eng, batch, ws, "dU2_16", B * Nk, H), cat("dU2"), R, "dU2", M, flips=F)
    close_rel(ws_bf16(eng, batch, ws, "dO2_16", B * Nk, H), cat("dO2"), R, "dO2", M, flips=F)
    d2 = ws_f32(eng, batch, ws, "delta2", B * 8 * 16).reshape(B, 8, 16)
    want_d2 = np.stack([(d["dO2"].reshape(Nk, 8, 32) * c["O2"].reshape(Nk, 8, 32)).sum(-1).T for d, c in zip(dbg, caches)])   # [B][8][Nk]
    # (row-dots and query-gradient sums are small differences of large terms: their own, wider bound)
    close_rel(d2[:, :, :Nk], want_d2, 5e-2, "delta2 = dO2 . O2", 1e-2, flips=2e-2)
    dqkv = ws_bf16(eng, batch, ws, "dQKV16", T, 3 * H)
    close_rel(dqkv[:, :H], cat("dQ"), R, "dQ", M, flips=F)
    close_rel(dqkv[:, H:2 * H], cat("dK2"), R, "dK2", M, flips=F)
    close_rel(dqkv[:, 2 * H:], cat("dV2"), R, "dV2", M, flips=F)
    close_rel(ws_f32(eng, batch, ws, "dKV", B * Nk * 2 * H).reshape(B * Nk, 2 * H), np.concatenate([cat("dKk"), cat("dVk")], axis=1), R, "dK | dV sums", M, flips=F)
    close_rel(ws_f32(eng, batch, ws, "dQ2acc", B * Nk * H).reshape(B * Nk, H), cat("dQ2"), 5e-2, "dQ2 sums", 1e-2, flips=2e-2)
    close_rel(ws_bf16(eng, batch, ws, "dQKVkg16", B * Nk, 3 * H), np.concatenate([cat("dQ2"), cat("dKk"), cat("dVk")], axis=1), R, "dQKV (KG rows)", M, flips=F)
    if not param_space:
        close_rel(ws_bf16(eng, batch, ws, "dR16", T, H), cat("dR"), R, "dR", M, flips=F)      # (formed below ~10 k packed rows only: above, the
        close_rel(ws_bf16(eng, batch, ws, "dG16", B * Nk, H), cat("dG"), R, "dG", M, flips=F)  # projections' weight gradients are taken in parameter space)
    num = den = 0.0
    rels = []
    for k, p in m.named_parameters():
        want = ref["raw_grads"][k].astype(np.float64); got = t2n(p.grad).astype(np.float64)
        num += ((got - want) ** 2).sum(); den += (want ** 2).sum()
        rels.append((np.sqrt(((got - want) ** 2).sum()) / max(np.sqrt((want ** 2).sum()), 1e-30), np.sqrt((want ** 2).sum()), k))
    rels.sort(reverse=True)
    total = np.sqrt(num / den)
    print("fused backward vs the bf16-operand oracle: global relative gradient error", total, "worst", [(f"{r:.4f}", f"{n:.2e}", k) for r, n, k in rels[:6]])
    assert not failures, "\n".join(failures)
    assert total < 2e-3, total
    gn = np.sqrt(den)
    assert all(r < 1e-2 for r, n, _ in rels if n > 1e-3 * gn), rels[:6]
    assert_attention_grad_blocks_close(got_grads, ref["raw_grads"], what=f"stage by stage, training={training} wide2={wide2} param_space={param_space}")


@pytest.mark.parametrize("training,B,ncls", [(False, 9, 2), (True, 16, 2), (True, 1, 2), (True, 6, 2), (True, 13, 2), (True, 3, 2), (True, 17, 2), (True, 40, 2), (True, 48, 2),
                                              (False, 33, 2), (True, 35, 5), (True, 11, 8)])
def test_one_launch_tail_matches_separate_launches(training, B, ncls, kg_real, fused_opts):
    """The per-sample tail as ONE launch of 64 co-resident blocks per group of 16 samples (misc.hip, tail_fused_kernel: split weights,
    three in-kernel all-reduces; B > 16: independent groups, the big weight gradients in one batched launch behind it) against the ten separate launches it replaces, on the same fused node-level kernels: outputs, loss terms,
    predictions and every parameter gradient.  Both tails compute in exact fp32; they differ in summation order only."""
    cfg = OP.full_cfg(dict(num_classes=ncls))
    m = make_model(cfg, 4, "bf16")
    m.train(training)
    eng = m._engine
    pool = NRS + [300, 77, 512, 40, 333, 9, 128]
    nrs = [pool[i % len(pool)] for i in range(B)]
    rg = np.concatenate([OP.make_rg(n, 128, seed=170 + i) for i, n in enumerate(nrs)])
    kg = np.stack([kg_real] * B)
    y, e, s = OP.make_labels(B, seed=15)
    batch = eng.make_batch(torch.from_numpy(rg).cuda(), nrs, torch.from_numpy(kg).cuda())
    res = []
    for mode in (-1, 0):
        fused_opts("tail17", mode)
        ws = eng.workspace(batch, private=True)
        ws.zero_()
        g = eng.ensure_flat_grads(attach=True)
        g.zero_()
        outs, terms, pred = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), training, 99, eng._gtab)
        torch.cuda.synchronize()
        res.append((t2n(outs), t2n(terms), t2n(pred), {k: t2n(p.grad).copy() for k, p in m.named_parameters()}))
        o_inf, _ = eng.forward_raw(batch, eng.workspace(batch, private=True), training, 99, inference=True)
        assert_close(t2n(o_inf), t2n(outs), 1e-6, 1e-5, "inference forward (one-launch tail, forward only) vs the training call")
    fused_opts("tail17", -1)
    (oa, ta, pa, ga), (ob, tb, pb, gb) = res
    assert_close(oa, ob, 2e-6, 1e-5, "outputs")
    assert_close(ta, tb, 2e-6, 1e-5, "loss terms")
    assert np.array_equal(pa, pb)
    for k in ga:
        scale = max(float(np.abs(gb[k]).max()), 1e-8)
        # node-level gradients pass through bf16 operands: a 1-ulp fp32 difference in d(mean H) can flip a bf16 rounding
        # (tail tensors: fp32 sums in another order -- a gradient that is a small difference of large terms moves by ~1e-4 of itself)
        tol = 3e-4 if (k.startswith(("mask_head", "instance_head", "edge_head", "score_head")) or "fusion_layer" in k or ".3." in k) else 4e-3
        assert float(np.abs(ga[k] - gb[k]).max()) <= tol * scale + 2e-7, (k, float(np.abs(ga[k] - gb[k]).max()), scale)


@pytest.mark.parametrize("nrs,nk,pseed", [([1], 1, 6), ([5, 700, 32], 16, 6), ([64] * 17, 13, 6), ([33, 31, 1, 2, 530, 96], 13, 6),
                                          ([33, 31, 1, 2, 530, 96], 13, 7), ([33, 31, 1, 2, 530, 96], 13, 8), ([1500, 17], 7, 6),
                                          ([420 + 5 * i for i in range(24)], 13, 6), ([128] * 3 + [127, 129, 256, 64, 192], 13, 6)])
def test_fused_training_step_shape_envelope(nrs, nk, pseed, fused_opts):
    _training_step_shape_envelope(nrs, nk, pseed, fused_opts, wide2=0)


@pytest.mark.parametrize("nrs,nk,pseed", [([5, 700, 32], 16, 6), ([33, 31, 1, 2, 530, 96], 13, 7), ([1500, 17], 7, 6), ([128] * 3 + [127, 129, 256, 64, 192], 13, 6),
                                          ([420 + 5 * i for i in range(24)], 13, 8)])
def test_fused_training_step_shape_envelope_64row_forward(nrs, nk, pseed, fused_opts):
    """The same envelope with the forward on 64-row half-blocks (fused_wide2.hip, saving + dropout variants) in front of the same
    backward kernels: same oracle, same bounds."""
    _training_step_shape_envelope(nrs, nk, pseed, fused_opts, wide2=1)


@pytest.mark.parametrize("nrs,nk,pseed", [([1], 1, 6), ([5, 700, 32], 16, 6), ([33, 31, 1, 2, 530, 96], 13, 7), ([1500, 17], 7, 6),
                                          ([128] * 3 + [127, 129, 256, 64, 192], 13, 6), ([64] * 17, 13, 6)])
def test_fused_training_step_shape_envelope_64row_backward_parameter_space(nrs, nk, pseed, fused_opts):
    """The same envelope on the schedule large batches run: 64-row forward, both backward halves on 64-row blocks (bwd1w_kernel, bwd2w_kernel
    + bwd2w_finish_kernel) and the projections' weight gradients in parameter space -- forced here at shapes that by size would not take
    it: one-node samples, Nk = 1 / 7 / 16, samples ending on tile boundaries, two samples in one 64-row block."""
    _training_step_shape_envelope(nrs, nk, pseed, fused_opts, wide2=2)


def _training_step_shape_envelope(nrs, nk, pseed, fused_opts, wide2):
    """Envelope of the fused BACKWARD (and of the one-launch tail where B <= 16): one-node samples, Nk = 1 / 7 / 16, samples
    that end exactly on a 32-, 64- or 128-row boundary, B = 17 (multi-launch tail behind fused node kernels), a 1500-node sample,
    24 samples with 11 460 rows (the weight-gradient launch's split-K ladder picks a 24-tile chunk: not a power of two) --
    against the train step of the oracle in its bf16-operand mode with the same dropout masks, at FIXED bounds: global relative
    gradient error < 0.2 %, every tensor that carries weight < 1 % (measured: 0.002-0.02 % and <= 0.2 %).  Tiny samples weigh single rows heavily, and with parameter
    seed 6 the six-sample case has head units whose pre-activation sits within bf16 noise of zero in three samples: against
    the reference-exact f32 oracle one such ReLU flip moves instance_head.0.bias by 18 % (tools/dev/dev_relu_flip.py); the bf16-operand
    oracle rounds what the kernels round and lands on the same side.  The f32 oracle still bounds the logits (north_star: 1e-3)."""
    fused_opts("wide2", min(wide2, 1)); fused_opts("wide2_bwd", min(wide2, 1))      # (1: forward AND the backward's first half on 64-row half-blocks)
    if wide2 == 2:
        fused_opts("param_space", 1)                                # (2: ... and the parameter-space second half)
    cfg = OP.full_cfg()
    m = make_model(cfg, pseed, "bf16").train()
    eng = m._engine
    B = len(nrs)
    rgl = [OP.make_rg(n, 128, seed=300 + i) for i, n in enumerate(nrs)]
    kg = np.stack([OP.make_kg(nk, 128, seed=400 + i) for i in range(B)])
    y, e, s = OP.make_labels(B, seed=21)
    dseed = 1234
    ref32, _ = FO.FusionOracle(cfg, OP.make_params(cfg, pseed)).forward_list(rgl, kg, training=True, seed=dseed)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rgl)).cuda(), list(nrs), torch.from_numpy(kg).cuda())
    ws = eng.workspace(batch, private=True)
    g = eng.ensure_flat_grads(attach=True)
    g.zero_()
    outs, terms, pred = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, dseed, eng._gtab)
    torch.cuda.synchronize()
    grads = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    assert np.isfinite(t2n(outs)).all() and all(np.isfinite(v).all() for v in grads.values())
    # (tail units whose pre-activation is within 5e-5 of the ReLU threshold may land on either side: helpers.py bounds how many)
    ref, near, flipped = oracle_step_at_relu_thresholds(
        lambda: bf16_oracle(cfg, OP.make_params(cfg, pseed), nrs, wide2 or sum(nrs) >= 57344),      # (by size training calls take the 64-row forward from 57 344 packed rows)
        lambda o: FO.train_step(o, FO.AdamW(o.p), rgl, kg, y, e, s, training=True, seed=dseed), grads)
    if near:
        print("tail units at the ReLU threshold (site, sample, unit, pre-activation):", near, "taken flipped:", flipped)
    assert_close(t2n(outs), outs6(ref32), 1e-3, 0, "outputs vs the f32 oracle")
    assert_close(t2n(outs), outs6(ref["outs"]), 5e-4, 0, "outputs vs the bf16-operand oracle")
    assert_close(t2n(terms), ref["loss_terms"], 2e-3, 1e-3, "loss terms")
    den = sum(float((ref["raw_grads"][k].astype(np.float64) ** 2).sum()) for k in grads)
    num = sum(float(((grads[k].astype(np.float64) - ref["raw_grads"][k]) ** 2).sum()) for k in grads)
    per = sorted(((float(np.sqrt(((grads[k].astype(np.float64) - ref["raw_grads"][k]) ** 2).sum() / max((ref["raw_grads"][k].astype(np.float64) ** 2).sum(), 1e-30))), k)
                  for k in grads if (ref["raw_grads"][k].astype(np.float64) ** 2).sum() > 1e-6 * den), reverse=True)
    total = float(np.sqrt(num / den))
    print(f"nrs={nrs[:6]} nk={nk} pseed={pseed}: global relative gradient error vs the bf16-operand oracle {total:.5f}; worst {per[0][1]} {per[0][0]:.4f}")
    assert total < 2e-3, (total, per[:4])
    assert per[0][0] < 1e-2, per[:4]
    assert_attention_grad_blocks_close(grads, ref["raw_grads"], what=f"nrs={nrs[:6]} nk={nk} pseed={pseed} wide2={wide2}",
                                       single_column=single_column_attentions(nrs, nk))
    # the same step with the projections' / in-projections' weight gradients taken in parameter space (bwd2p_kernel + unfold_kernel;
    # by size from 10 240 packed rows, forced here -- or forced OFF where the size rule took it above), against the same oracle step
    fused_opts("param_space", 0 if sum(nrs) >= 10240 else 1)
    g.zero_()
    outs2, _, _ = eng.train_raw(batch, eng.workspace(batch, private=True), torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, dseed, eng._gtab)
    torch.cuda.synchronize()
    fused_opts("param_space", -1)
    grads2 = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    assert_close(t2n(outs2), t2n(outs), 1e-6, 1e-6, "outputs do not depend on the backward's form")
    num2 = sum(float(((grads2[k].astype(np.float64) - ref["raw_grads"][k]) ** 2).sum()) for k in grads2)
    per2 = sorted(((float(np.sqrt(((grads2[k].astype(np.float64) - ref["raw_grads"][k]) ** 2).sum() / max((ref["raw_grads"][k].astype(np.float64) ** 2).sum(), 1e-30))), k)
                   for k in grads2 if (ref["raw_grads"][k].astype(np.float64) ** 2).sum() > 1e-6 * den), reverse=True)
    print(f"   other form of the backward: global {float(np.sqrt(num2 / den)):.5f}; worst {per2[0][1]} {per2[0][0]:.4f}")
    assert float(np.sqrt(num2 / den)) < 2e-3, per2[:4]
    assert per2[0][0] < 1e-2, per2[:4]
    assert_attention_grad_blocks_close(grads2, ref["raw_grads"], what=f"nrs={nrs[:6]} nk={nk} pseed={pseed} wide2={wide2}, other form of the backward",
                                       single_column=single_column_attentions(nrs, nk))


@pytest.mark.parametrize("B,ncls", [(1, 2), (17, 2), (32, 2), (33, 3), (100, 2)])
def test_wide_tail_matches_separate_launches(B, ncls, kg_real, fused_opts):
    """The per-sample tail of wide-tile inference calls as ONE launch (csrc/tail_wide.hip: 32 samples per block, two-plane bf16
    operands, three MFMA products per term) against the five fp32 GEMM launches it replaces, on the same node-level kernels, and
    against the oracle.  The two tails differ by the dropped x_lo * W_lo term (2^-18 relative) and summation order."""
    cfg = OP.full_cfg(dict(num_classes=ncls))
    m = make_model(cfg, 5, "bf16").eval()
    eng = m._engine
    rs = np.random.RandomState(B)
    nrs = [int(x) for x in rs.randint(1, 200, size=B)]
    rg = [OP.make_rg(n, 128, seed=500 + i) for i, n in enumerate(nrs)]
    kg = np.stack([kg_real * (1.0 + 0.01 * (i % 7)) for i in range(B)]).astype(np.float32)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), nrs, torch.from_numpy(kg).cuda())
    fused_opts("fused_rt", 4)
    res = []
    for mode in (1, 0):                                     # (1: the two-plane tail also where the size rule prefers the grouped fp32 tail, B <= 32)
        fused_opts("tailw", mode)
        o, _ = eng.forward_raw(batch, eng.workspace(batch, private=True), False, 7, inference=True, cache_shadows=False)
        res.append(t2n(o))
    assert np.isfinite(res[0]).all()
    assert_close(res[0], res[1], 2e-5, 1e-5, "one-launch wide tail vs five launches")
    ref, _ = FO.FusionOracle(cfg, OP.make_params(cfg, 5)).forward_list(rg, kg)
    assert_close(res[0], outs6(ref), 1e-3, 0, "wide tail vs oracle")


def test_large_batch_training_takes_the_wide_front_half(kg_real, fused_opts):
    """Training calls with at least 4 * 32 * 224 rows run the front half on 128-row blocks (fused_wide.hip, front8_kernel), past 64
    samples the per-sample tail's forward and input-gradient chain on two-plane MFMA launches (tail_wide.hip), and keep the
    32-row back half: the same bf16 tensors leave the front launch, so outputs and loss terms agree to rounding and every parameter
    gradient to a few 1e-4 of its tensor against the all-32-row schedule (fused_rt = 0) on the same masks."""
    fused_opts("wide2", 0)      # (by size a batch like this now runs its forward on the 64-row half-blocks -- tests/test_hip_large_batch.py holds that
                                # to the oracle; the wide front half + 32-row back half is what training calls of 10 240 .. 13 311 rows take)
    cfg = OP.full_cfg()
    m = make_model(cfg, 4, "bf16")
    m.train()
    eng = m._engine
    B = 70
    nrs = [380 + 3 * (i % 50) for i in range(B)]              # T = 31 k rows
    rg = np.concatenate([OP.make_rg(n, 128, seed=900 + i) for i, n in enumerate(nrs)])
    kg = np.stack([kg_real] * B)
    y, e, s = OP.make_labels(B, seed=21)
    batch = eng.make_batch(torch.from_numpy(rg).cuda(), nrs, torch.from_numpy(kg).cuda())
    res = []
    for rt in (-1, 0):
        fused_opts("fused_rt", rt)
        ws = eng.workspace(batch, private=True)
        ws.zero_()
        g = eng.ensure_flat_grads(attach=True)
        g.zero_()
        outs, terms, pred = eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, 41, eng._gtab)
        torch.cuda.synchronize()
        res.append((t2n(outs), t2n(terms), {k: t2n(p.grad).copy() for k, p in m.named_parameters()}))
    fused_opts("fused_rt", -1)
    # the same wide-front step with the tail's backward on its four fp32 GEMM launches instead of the two-plane launch: the tail
    # parameters' gradients differ by the planes' 2^-17 and by summation order only
    fused_opts("tailw_bwd", 0)
    ws = eng.workspace(batch, private=True)
    ws.zero_()
    g.zero_()
    eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, 41, eng._gtab)
    torch.cuda.synchronize()
    fused_opts("tailw_bwd", -1)
    gc = {k: t2n(p.grad).copy() for k, p in m.named_parameters()}
    for k in gc:
        if k.startswith(("mask_head", "instance_head", "edge_head", "score_head")) or "fusion_layer" in k or ".3." in k:
            scale = max(float(np.abs(gc[k]).max()), 1e-8)
            assert float(np.abs(res[0][2][k] - gc[k]).max()) <= 3e-4 * scale + 2e-7, (k, float(np.abs(res[0][2][k] - gc[k]).max()), scale)
    (oa, ta, ga), (ob, tb, gb) = res
    assert np.isfinite(oa).all()
    assert_close(oa, ob, 2e-4, 1e-4, "outputs")
    assert_close(ta, tb, 2e-4, 1e-4, "loss terms")
    num = sum(float(((ga[k].astype(np.float64) - gb[k]) ** 2).sum()) for k in ga)
    den = sum(float((gb[k].astype(np.float64) ** 2).sum()) for k in gb)
    assert np.sqrt(num / den) < 1e-3, np.sqrt(num / den)


@pytest.mark.parametrize("nrs", [[300, 77, 512, 40, 333, 9, 128, 1], [420 + 5 * i for i in range(40)]])
def test_weight_gradients_on_128x256_tiles_match_the_64x128_kernel(nrs, kg_real, fused_opts):
    """The weight-gradient launch of long contractions (gemm16.hip, gemm16_tnbig_kernel: 128 x 256 tiles on 8 waves, taken by size at
    K >= 40 000 packed rows and forced here at small K) against the 64 x 128 kernel on the same operands: the same products in
    another split-K and fp32-atomic order."""
    cfg = OP.full_cfg()
    m = make_model(cfg, 4, "bf16")
    m.train()
    eng = m._engine
    B = len(nrs)
    rg = np.concatenate([OP.make_rg(n, 128, seed=700 + i) for i, n in enumerate(nrs)])
    kg = np.stack([kg_real] * B)
    y, e, s = OP.make_labels(B, seed=33)
    batch = eng.make_batch(torch.from_numpy(rg).cuda(), nrs, torch.from_numpy(kg).cuda())
    res = []
    for big in (1, 0):
        fused_opts("tn_big", big)
        ws = eng.workspace(batch, private=True)
        ws.zero_()
        g = eng.ensure_flat_grads(attach=True)
        g.zero_()
        eng.train_raw(batch, ws, torch.from_numpy(y), torch.from_numpy(e), torch.from_numpy(s), True, 43, eng._gtab)
        torch.cuda.synchronize()
        res.append({k: t2n(p.grad).astype(np.float64) for k, p in m.named_parameters()})
    fused_opts("tn_big", -1)
    ga, gb = res
    for k in ga:
        scale = max(float(np.abs(gb[k]).max()), 1e-8)
        assert np.isfinite(ga[k]).all(), k
        # (the two steps differ upstream too: fp32 atomics in the backward kernels land in another order from run to run and flip
        # bf16 roundings of the gradient operands -- the bound is that effect's, a tile-indexing error would be O(scale))
        assert float(np.abs(ga[k] - gb[k]).max()) <= 2e-3 * scale + 1e-7, (k, float(np.abs(ga[k] - gb[k]).max()), scale)
