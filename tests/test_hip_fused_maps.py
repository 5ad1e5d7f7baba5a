"""Attention maps on the fused inference schedule (CAMO_FWD_FUSED_MAPS, csrc/attn_maps.hip) against the oracle.  Needs an MI355X.

Yardstick: the numpy oracle, never another HIP schedule.  Tolerances are computed per case on the CPU from the two oracles:
E = max |map(bf16-operand oracle) - map(f32 oracle)| is what bf16 operands cost by the model; the kernel must be nearer to its
model than the model is to the truth (<= E) and within 2 E of the f32 oracle (triangle inequality).  Two parameter sets: the
seed-0 one (maps nearly uniform) and a peaked one built here (SHARP: every head's query / key projection a scaled copy of head
0's, x 32 -- the f32 oracle's maps then have rows with a maximum >= 0.5 in both directions, asserted before the kernel is looked
at; the heads' temperatures differ, so a wrong head order changes the result).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import assert_close
from oracle import fusion_oracle as FO
from oracle import params as OP
from test_hip_parity import make_model, outs6, t2n

pytestmark = pytest.mark.gpu

REAL = [303, 481, 500, 530]
SMALL = [1, 31, 32, 33, 64, 65]


def sharp_params(cfg):
    p = {k: np.array(v, np.float32) for k, v in OP.make_params(cfg, 0).items()}
    H = cfg["hidden_dim"]
    for a in ("cross_attn_rg2kg", "cross_attn_kg2rg"):
        W, b = p[f"fusion.{a}.in_proj_weight"], p[f"fusion.{a}.in_proj_bias"]
        for blk in (0, 1):                               # query rows, key rows
            for h in range(8):
                g = np.float32(32.0 * ((0.65 + 0.1 * h) if blk == 0 else 1.0))
                W[blk * H + 32 * h: blk * H + 32 * h + 32] = W[blk * H: blk * H + 32] * (g if h else np.float32(1))
                b[blk * H + 32 * h: blk * H + 32 * h + 32] = b[blk * H: blk * H + 32] * (g if h else np.float32(1))
            g0 = np.float32(32.0 * (0.65 if blk == 0 else 1.0))
            W[blk * H: blk * H + 32] *= g0; b[blk * H: blk * H + 32] *= g0
    return p


PARAMS = {"seed0": lambda cfg: OP.make_params(cfg, 0), "sharp": sharp_params}


def batch_inputs(nrs, nk, kg_real, seed=0):
    rg = [OP.make_rg(n, 128, seed=900 + seed + i) for i, n in enumerate(nrs)]
    if nk == 13:
        kg = np.stack([kg_real * np.float32(1.0 + 0.03 * (i % 5)) for i in range(len(nrs))]).astype(np.float32)
    else:
        kg = np.stack([OP.make_kg(nk, 128, seed=70 + seed + i) for i in range(len(nrs))])
    return rg, kg


def fused_plan(m, nrs, nk, fused_maps=True, training=False):
    from camouflage_multimodal_amd import _lib
    eng = m._engine
    p = _lib.CamoPlan()
    flags = _lib.FWD_INFERENCE | _lib.FLAG_ATTN_MAPS | (_lib.FWD_FUSED_MAPS if fused_maps else 0)
    _lib.check(_lib.lib().camo_debug_plan(C.byref(eng.dims), 3, len(nrs), sum(nrs), nk, max(nrs), _lib.PREC_BF16, flags, _lib.CALL_FORWARD, -1,
                                          C.byref(p)), "camo_debug_plan")
    return p


def run(m, rg, nrs, kg, fused=True, attention=True):
    with torch.no_grad():
        o = m.forward_packed(torch.from_numpy(np.concatenate(rg)).cuda(), list(nrs), torch.from_numpy(kg).cuda(), return_attention=attention,
                             fused_attention=fused)
    torch.cuda.synchronize()
    outs = np.concatenate([t2n(v) for v in o[:4]], axis=1)
    if not attention:
        return outs, None, None
    return outs, [t2n(a) for a in o[4]["rg2kg"]], [t2n(a) for a in o[4]["kg2rg"]]


CASES = [
    ("real_B4", REAL, 13), ("real_B1_500", [500], 13), ("small_B6", SMALL, 13), ("nr2048_B1", [2048], 13),
    ("nk1_B3", [303, 33, 1], 1), ("nk16_B3", [530, 65, 32], 16),
    ("B16", REAL * 4, 13), ("B24_T10884", REAL * 6, 13),
]


@pytest.mark.parametrize("pname", ["seed0", "sharp"])
@pytest.mark.parametrize("name,nrs,nk", CASES, ids=[c[0] for c in CASES])
def test_maps_against_both_oracles(name, nrs, nk, pname, kg_real):
    cfg = OP.full_cfg()
    prm = PARAMS[pname](cfg)
    rg, kg = batch_inputs(nrs, nk, kg_real)
    ref32, _ = FO.FusionOracle(cfg, prm).forward_list(rg, kg)
    ref16, _ = FO.FusionOracle(cfg, prm, bf16_operands=True).forward_list(rg, kg)
    if pname == "sharp" and nk > 1:
        # the comparison must mean something: peaked maps in both directions, by the f32 oracle
        assert max(a.max() for a in ref32["attn_rg2kg"]) >= 0.5 and max(a.max() for a in ref32["attn_kg2rg"] if a.shape[1] > 1) >= 0.5
    m = make_model(cfg, 0, "bf16", params=prm).eval()
    p = fused_plan(m, nrs, nk)
    assert p.nodes == 3 and p.maps == 1, "the case must run the fused schedule + the maps launch"
    assert (sum(nrs) >= 10240) == (p.front == 1)
    outs, a1, a2 = run(m, rg, nrs, kg)
    if pname == "seed0":
        assert_close(outs, outs6(ref32), 1e-3, 0, "outputs vs the f32 oracle")
    worst = {}
    for key, got in (("attn_rg2kg", a1), ("attn_kg2rg", a2)):
        E = max(float(np.abs(ref16[key][b] - ref32[key][b]).max()) for b in range(len(nrs)))
        d16 = max(float(np.abs(got[b] - ref16[key][b]).max()) for b in range(len(nrs)))
        d32 = max(float(np.abs(got[b] - ref32[key][b]).max()) for b in range(len(nrs)))
        worst[key] = (E, d16, d32)
        print(f"fused maps {name} {pname} {key}: E {E:.3e}  |hip - bf16 oracle| {d16:.3e}  |hip - f32 oracle| {d32:.3e}")
    for b, n in enumerate(nrs):
        assert a1[b].shape == (n, nk) and a2[b].shape == (nk, n)
        assert np.isfinite(a1[b]).all() and np.isfinite(a2[b]).all()
        assert_close(a1[b].sum(1), np.ones(n), 1e-5, 0, "rg2kg rows sum to 1")
        assert_close(a2[b].sum(1, dtype=np.float64), np.ones(nk), 2.0 ** -8, 0, "kg2rg rows sum to 1")
    for key, (E, d16, d32) in worst.items():
        assert d16 <= E, f"{key}: |hip - bf16 oracle| {d16:.3e} > E {E:.3e}"
        assert d32 <= 2 * E, f"{key}: |hip - f32 oracle| {d32:.3e} > 2 E {2 * E:.3e}"


@pytest.mark.parametrize("pname", ["seed0", "sharp"])
def test_kg_permutation_permutes_map_columns(pname, kg_real):
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16", params=PARAMS[pname](cfg)).eval()
    nrs = [303, 33, 65]
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=5)
    perm = np.random.RandomState(3).permutation(13)
    _, a1, a2 = run(m, rg, nrs, kg)
    _, b1, b2 = run(m, rg, nrs, np.ascontiguousarray(kg[:, perm]))
    for b in range(len(nrs)):
        # (a key's probability does not depend on its position; the row's softmax sums its 13 terms in another order)
        assert_close(b1[b], a1[b][:, perm], 2e-6, 0, "rg2kg columns")
        assert_close(b2[b], a2[b][perm], 2e-6, 0, "kg2rg rows")


def test_packed_batch_equals_singles(kg_real):
    """Seed-0 parameters, 2e-6: the bound and the parameters of test_hip_parity.py's packed-vs-singles test."""
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    nrs = REAL + SMALL
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=11)
    _, a1, a2 = run(m, rg, nrs, kg)
    worst = [0.0, 0.0]
    for b in range(len(nrs)):
        _, s1, s2 = run(m, [rg[b]], [nrs[b]], kg[b:b + 1])
        worst = [max(worst[0], float(np.abs(a1[b] - s1[0]).max())), max(worst[1], float(np.abs(a2[b] - s2[0]).max()))]
    print(f"fused maps packed vs singles: rg2kg {worst[0]:.3e}  kg2rg {worst[1]:.3e} (bound 2e-6)")
    assert worst[0] <= 2e-6 and worst[1] <= 2e-6


# what the fused forward leaves per row in the workspace: each element has ONE writer and a fixed summation order, so these are
# reproducible bit for bit (unlike the pooled per-sample sums behind them, which are accumulated with fp32 atomics)
ROW_TENSORS_FRONT = (("R16", "rg", 512), ("Q16", "rg", 512), ("KV2_16", "rg", 1024), ("G16", "kg", 512), ("Q2_16", "kg", 512), ("KV16", "kg", 1024))
ROW_TENSORS_BACK = (("O16", "rg", 512), ("Y16", "rg", 512), ("XH16", "rg", 512), ("mask1", "rg", 64),
                    ("O2_16", "kg", 512), ("Y2_16", "kg", 512), ("XH2_16", "kg", 512), ("mask2", "kg", 64))
# fp32 1/std per row: its cross-wave sum has no fixed order (two plain calls differ in the last bit): compared to 1e-6 relative
ROW_STATS = (("rstd1", "rg"), ("rstd2", "kg"))


def _raw_call(eng, batch, maps, save):
    """One inference call into a zeroed private workspace (weight shadows there too) -> (workspace, outs, maps or None)."""
    eng.set_option("fused_save", int(save))
    try:
        ws = eng.workspace(batch, private=True)
        ws.zero_()
        outs, attn = eng.forward_raw(batch, ws, False, 77, want_attention=maps, inference=True, cache_shadows=False, fused_maps=maps)
        torch.cuda.synchronize()
    finally:
        eng.set_option("fused_save", 0)
    return ws, t2n(outs), attn


def _ws_bytes(eng, batch, ws, name, nbytes):
    from camouflage_multimodal_amd import _lib
    off = _lib.lib().camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
    assert off >= 0, name
    return ws[off:off + nbytes].cpu().numpy().copy()


@pytest.mark.parametrize("nrs", [[1, 31, 32, 17], REAL, REAL * 4], ids=["one_tile_samples", "real_B4", "real_B16"])
def test_forward_undisturbed_below_the_switch(nrs, kg_real):
    """Below 10 240 packed rows a maps call and a plain inference call plan the same node-level kernels and the same tail: the lse2
    store and the maps launch must not disturb the forward.
      * Bit for bit where the forward is reproducible: every per-row tensor it leaves in the workspace (front half: R16, Q16,
        KV2_16, G16, Q2_16, KV16; back half, written under the fused_save hook: attention outputs, LayerNorm outputs and inputs,
        ReLU masks of both streams; the fp32 1/std per row to 1e-6 relative) and the KG->RG softmax statistics lse2 -- which the maps call WITHOUT the hook must
        store exactly as a saving call does.
      * The six outputs pass through per-sample sums pooled with fp32 atomics (several adds per column even within one 32-row
        tile; the one-launch tail all-reduces the same way), so two plain calls on the same inputs differ in their last bits:
        measured on an MI355X up to 6e-8.  Bound: 1e-6 abs, what test_hip_fused.py allows the same forward run twice (its
        inference call against the training call's forward)."""
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    eng = m._engine
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=21)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), nrs, torch.from_numpy(kg).cuda())
    rows = {"rg": batch.T, "kg": batch.B * 13}
    lse_bytes = batch.B * 8 * 16 * 2 * 4
    ws_ps, o_ps, _ = _raw_call(eng, batch, maps=False, save=True)        # plain call, saved set written
    ws_ms, o_ms, a_ms = _raw_call(eng, batch, maps=True, save=True)      # maps call, saved set written
    ws_m, o_m, a_m = _raw_call(eng, batch, maps=True, save=False)        # maps call as the product makes it
    ws_p, o_p, _ = _raw_call(eng, batch, maps=False, save=False)
    for name, side, width in ROW_TENSORS_FRONT + ROW_TENSORS_BACK:
        want = _ws_bytes(eng, batch, ws_ps, name, rows[side] * width)
        assert want.any(), f"{name}: the saving call left nothing to compare"
        assert np.array_equal(_ws_bytes(eng, batch, ws_ms, name, rows[side] * width), want), f"{name}: maps call != plain call (saved set)"
    ws_ps2, _, _ = _raw_call(eng, batch, maps=False, save=True)          # (a second plain call: what "reproducible" means here)
    for name, side in ROW_STATS:
        want = _ws_bytes(eng, batch, ws_ps, name, rows[side] * 4).view(np.float32)
        again = _ws_bytes(eng, batch, ws_ps2, name, rows[side] * 4).view(np.float32)
        got = _ws_bytes(eng, batch, ws_ms, name, rows[side] * 4).view(np.float32)
        print(f"fused maps {name}: plain vs plain max rel {np.abs(again / want - 1).max():.2e}, maps vs plain {np.abs(got / want - 1).max():.2e}")
        assert_close(got, want, 0, 1e-6, name)
    for name, side, width in ROW_TENSORS_FRONT + ROW_TENSORS_BACK:
        assert np.array_equal(_ws_bytes(eng, batch, ws_ps2, name, rows[side] * width), _ws_bytes(eng, batch, ws_ps, name, rows[side] * width)), name
    for name, side, width in ROW_TENSORS_FRONT:
        want = _ws_bytes(eng, batch, ws_ps, name, rows[side] * width)
        for what, ws in (("maps call", ws_m), ("plain call", ws_p)):
            assert np.array_equal(_ws_bytes(eng, batch, ws, name, rows[side] * width), want), f"{name}: {what} without the hook"
    lse = _ws_bytes(eng, batch, ws_ps, "lse2", lse_bytes)
    assert lse.any()
    assert np.array_equal(_ws_bytes(eng, batch, ws_ms, "lse2", lse_bytes), lse)
    assert np.array_equal(_ws_bytes(eng, batch, ws_m, "lse2", lse_bytes), lse), "lse2 of a maps call != lse2 of a saving call"
    assert not _ws_bytes(eng, batch, ws_p, "lse2", lse_bytes).any(), "a plain inference call stores no lse2, as before"
    # the maps themselves have one writer per element: the same with and without the hook
    for x, y in zip(a_ms, a_m):
        assert torch.equal(x, y)
    worst = max(float(np.abs(o - o_p).max()) for o in (o_ps, o_ms, o_m))
    print(f"fused maps outputs B={len(nrs)} T={sum(nrs)}: max |outputs - plain call's| over the three other calls {worst:.3e} (bound 1e-6)")
    assert worst <= 1e-6


def test_forward_outputs_agree_above_the_switch(kg_real):
    """From 10 240 packed rows the plain call runs the RG rows' one-launch forward (folded in-projection) and the maps call the
    wide front half + the 32-row back half: the bound test_size_switches.py uses across that switch (4e-4)."""
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    nrs = REAL * 6
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=31)
    plain, _, _ = run(m, rg, nrs, kg, attention=False)
    fused, _, _ = run(m, rg, nrs, kg)
    assert_close(fused, plain, 4e-4, 0, "maps call vs plain call, T >= 10 240")


def _prof(fn):
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    _lib.check(L.camo_prof_begin(256), "camo_prof_begin")
    fn()
    ms, n, fl = C.c_double(), C.c_int32(), C.c_double()
    _lib.check(L.camo_prof_end(C.byref(ms), C.byref(n), C.byref(fl)), "camo_prof_end")
    kinds = {}
    for kind in range(10):
        _lib.check(L.camo_prof_kind(kind, C.byref(ms), C.byref(n), C.byref(fl)), "camo_prof_kind")
        kinds[kind] = int(n.value)
    return kinds


def test_second_call_reuses_the_shadows(kg_real):
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    nrs = REAL
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=41)
    first = _prof(lambda: run(m, rg, nrs, kg))
    second = _prof(lambda: run(m, rg, nrs, kg))
    assert first[7] >= 1 and first[8] == 1, first            # weight shadows (+ fold) built; ONE attention launch: the maps kernel
    assert second[7] == 0 and second[8] == 1, second         # no shadow launch
    assert second[1] == 1 and second[2] == 1 and sum(second.values()) == 4, second     # front, back, maps, one-launch tail
    assert m._engine.shadows_current()
    # ... and a plain inference call after it still finds them current (3 launches)
    third = _prof(lambda: run(m, rg, nrs, kg, attention=False))
    assert third[7] == 0 and sum(third.values()) == 3, third


def test_training_mode_with_dropout_drops_the_flag(kg_real):
    """In training mode the reference returns the maps after attention dropout: the flag is dropped, today's schedule runs."""
    cfg = OP.full_cfg(dict(dropout=0.3))
    res = []
    for fused in (False, True):
        torch.manual_seed(1234)
        m = make_model(cfg, 0, "bf16").train()
        rg, kg = batch_inputs(REAL, 13, kg_real, seed=51)
        res.append(run(m, rg, REAL, kg, fused=fused))
    # (the outputs pass through pooled sums accumulated with fp32 atomics: two runs of the same call agree to their order -- 1e-6 abs
    # as in test_forward_undisturbed_below_the_switch; everything with one writer per element is compared bit for bit below)
    print(f"fused maps training-mode call: max |outputs with flag - without| {np.abs(res[0][0] - res[1][0]).max():.3e} (bound 1e-6)")
    assert np.abs(res[0][0] - res[1][0]).max() <= 1e-6
    for b in range(len(REAL)):                       # the maps have one writer per element: bit for bit, dropped entries included
        assert np.array_equal(res[0][1][b], res[1][1][b]) and np.array_equal(res[0][2][b], res[1][2][b])
    assert any((a == 0).any() for a in res[1][1]), "attention dropout must show in the maps of a training-mode call"


@pytest.mark.parametrize("nrs", [[33, 1, 500], REAL * 6], ids=["small", "T10884"])
def test_guards_around_the_map_buffers(nrs, kg_real):
    """Raw call with poisoned guard bands in front of and behind both [T, Nk] map buffers."""
    from camouflage_multimodal_amd import _lib
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    eng = m._engine
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=61)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), nrs, torch.from_numpy(kg).cuda())
    T, Nk, G = batch.T, 13, 4096
    ws = eng.workspace(batch, private=True)
    outs = torch.empty(batch.B, 6, device="cuda")
    POISON = -12345.0
    bufs = [torch.full((G + T * Nk + G,), POISON, device="cuda") for _ in range(2)]
    a = [b[G:G + T * Nk] for b in bufs]
    sh = eng.shadow_buffer()
    state = C.c_int32(0)
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    rc = _lib.lib().camo_forward_cached(C.byref(eng.dims), eng._ptab, _ptr(batch.rg), _ptr(batch.offsets), _ptr(batch.desc), _ptr(batch.kg),
                                        batch.B, batch.T, batch.Nk, batch.max_nr, _ptr(ws), ws.numel(), _ptr(outs), _ptr(a[0]), _ptr(a[1]), 0, 7, _lib.PREC_BF16,
                                        _lib.FWD_INFERENCE | _lib.FWD_FUSED_MAPS, _ptr(sh), 0, C.byref(state), _stream_ptr(eng.device))
    _lib.check(rc, "camo_forward_cached")
    torch.cuda.synchronize()
    assert state.value == 1, "a maps call with a shadow buffer keeps its shadows there"
    for b in bufs:
        h = b.cpu().numpy()
        assert (h[:G] == POISON).all() and (h[-G:] == POISON).all(), "guard bands touched"
        body = h[G:-G]
        assert np.isfinite(body).all() and (body >= 0).all() and (body <= 1.0 + 1e-6).all() and (body != POISON).all()


@pytest.mark.parametrize("which", [0, 1], ids=["rg2kg_only", "kg2rg_only"])
def test_one_map_pointer(which, kg_real):
    """camo_forward with ONE map pointer and the flag: that map equals the two-pointer call's bit for bit, guards intact."""
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    cfg = OP.full_cfg()
    m = make_model(cfg, 0, "bf16").eval()
    eng = m._engine
    nrs = [33, 1, 500, 64]
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=71)
    batch = eng.make_batch(torch.from_numpy(np.concatenate(rg)).cuda(), nrs, torch.from_numpy(kg).cuda())
    _, _, both = _raw_call(eng, batch, maps=True, save=False)
    T, Nk, G, POISON = batch.T, 13, 1024, -12345.0
    buf = torch.full((G + T * Nk + G,), POISON, device="cuda")
    a = buf[G:G + T * Nk]
    ptrs = [None, None]
    ptrs[which] = _ptr(a)
    ws = eng.workspace(batch, private=True)
    outs = torch.empty(batch.B, 6, device="cuda")
    rc = _lib.lib().camo_forward(C.byref(eng.dims), eng._ptab, _ptr(batch.rg), _ptr(batch.offsets), _ptr(batch.desc), _ptr(batch.kg), batch.B, batch.T,
                                 batch.Nk, batch.max_nr, _ptr(ws), ws.numel(), _ptr(outs), ptrs[0], ptrs[1], 0, 77, _lib.PREC_BF16,
                                 _lib.FWD_INFERENCE | _lib.FWD_FUSED_MAPS, _stream_ptr(eng.device))
    _lib.check(rc, "camo_forward")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:G] == POISON).all() and (h[-G:] == POISON).all(), "guard bands touched"
    assert np.array_equal(h[G:-G].reshape(T, Nk), t2n(both[which]))


def test_maps_on_the_128_row_front_half(kg_real):
    """T >= 28 672 packed rows: front = wide:4 (128-row blocks), the 32-row back half, five tail launches.  60 samples; the first,
    the last and two in the middle against both oracles under the bound of test_maps_against_both_oracles."""
    cfg = OP.full_cfg()
    prm = OP.make_params(cfg, 0)
    nrs = [REAL[i % 4] + 27 * (i % 3) for i in range(60)]
    assert sum(nrs) >= 28672
    rg, kg = batch_inputs(nrs, 13, kg_real, seed=81)
    m = make_model(cfg, 0, "bf16").eval()
    p = fused_plan(m, nrs, 13)
    assert p.maps == 1 and p.front == 1 and p.front_rt == 4 and p.back == 0
    outs, a1, a2 = run(m, rg, nrs, kg)
    assert np.isfinite(outs).all()
    for b in (0, 22, 41, 59):
        base = sum(nrs[:b])
        r32, _ = FO.FusionOracle(cfg, prm).forward_sample(rg[b], kg[b], row_base=base, b_index=b)
        r16, _ = FO.FusionOracle(cfg, prm, bf16_operands=True).forward_sample(rg[b], kg[b], row_base=base, b_index=b)
        for key, got in (("attn_rg2kg", a1[b]), ("attn_kg2rg", a2[b])):
            E = float(np.abs(r16[key] - r32[key]).max())
            d16, d32 = float(np.abs(got - r16[key]).max()), float(np.abs(got - r32[key]).max())
            print(f"fused maps wide:4 sample {b} {key}: E {E:.3e}  |hip - bf16 oracle| {d16:.3e}  |hip - f32 oracle| {d32:.3e}")
            assert d16 <= E and d32 <= 2 * E, (b, key, E, d16, d32)
