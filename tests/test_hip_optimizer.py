"""sumsq_kernel, clip_adamw_kernel and adamw_shadow_kernel (csrc/misc.hip) against the float64 reference
oracle/f64_refs.adamw_f64, called through the C ABI on buffers the test owns.  Needs an MI355X.

Every element of p, g, m and v must sit under its own bound -- 2 x the first-order propagation of one rounding per float32
operation of adamw_update and of the clip coefficient + 1 ulp (written out next to the formula in adamw_f64; the sum of squares
carries (ceil(n / 65 536) + 16) u).  No element is exempted: the gradient is an input here, so an element whose gradient is
rounding noise has a definite answer like any other.  tests/test_f64_refs.py shows on the CPU that eight plausible errors (no /
L2 / late decay, eps inside the root, bc2 without the root, step - 1, no clamp, unclipped first moment) exceed these bounds 10 x
on the n = 1023 cross run below.

Paths, reached by size and address: the float4 body and the scalar tail (n % 4 != 0), the unaligned branch (all four buffers
offset by one float: n4 = 0), the grid-stride second pass (n > 1024 blocks x 256 threads x 4 elements), and in the shadow kernel
the tile blocks, the long-range blocks and the one-block short ranges, all away from zero moments.

Behaviour found and left as it is: a gradient whose float32 sum of squares overflows (norm > ~1.8e19) while its float64 norm is
finite makes the step a no-op (the Inf-norm skip) where torch would clip it to max_norm; the gradients here stop at 1e3.

Largest observed error / bound (MI355X):  
  clip_adamw_kernel, n = 1023 cross                 sumsq 0.04, grad_norm 0.07, p 0.22, g 0.12, m 0.29, v 0.31
  sumsq_kernel / clip_adamw_kernel, sizes           sumsq 0.03, grad_norm 0.05, p 0.22, g 0.07, m 0.33, v 0.33 (aligned and unaligned alike)
  five carried steps                                sumsq 0.04, grad_norm 0.05, p 0.22, g 0.06, m 0.32, v 0.35
  adamw_shadow_kernel (bit-identical to the above)  sumsq 0.03, grad_norm 0.03, p 0.21, g 0.05, m 0.33, v 0.33
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import f64_cases as FC
from oracle import f64_refs as R
from oracle import params as OP

pytestmark = pytest.mark.gpu

PAD = 64                      # canary floats on each side (256 bytes: the data stays 16-byte aligned behind them)
CANARY = -4321.5
SUMSQ_FLOATS = 257


class Buffers:
    """p, g, m, v and the 257-float norm scratch on the device, each between canaries; ``offset`` floats past 16-byte alignment."""

    def __init__(self, p, g, m, v, offset=0):
        self.n = n = len(p)
        self.raw, self.t = {}, {}
        for k, a in (("p", p), ("g", g), ("m", m), ("v", v), ("ss", np.zeros(SUMSQ_FLOATS, np.float32))):
            off = 0 if k == "ss" else offset
            raw = torch.full((len(a) + 2 * PAD + off,), CANARY, dtype=torch.float32, device="cuda")
            view = raw[PAD + off:PAD + off + len(a)]
            view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
            assert view.data_ptr() % 16 == 4 * off
            self.raw[k], self.t[k] = raw, view
        self.offset = offset

    def ptr(self, k):
        return C_.c_void_p(self.t[k].data_ptr())

    def step(self, h, step, zero_grads):
        from camouflage_multimodal_amd import _lib
        L = _lib.lib()
        st = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.camo_grad_sumsq(self.ptr("g"), self.n, self.ptr("ss"), st), "camo_grad_sumsq")
        _lib.check(L.camo_clip_adamw(self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), self.n, self.ptr("ss"), h["max_norm"],
                                     h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, zero_grads, st), "camo_clip_adamw")
        torch.cuda.synchronize()

    def get(self, k):
        return self.t[k].cpu().numpy().copy()

    def canaries_intact(self):
        for k, raw in self.raw.items():
            b = raw.cpu().numpy(); lo = PAD + (0 if k == "ss" else self.offset); n = len(self.t[k])
            if not ((b[:lo] == np.float32(CANARY)).all() and (b[lo + n:] == np.float32(CANARY)).all()):
                return False
        return True


WORST = {}


def _ratio(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{what}: non-finite value"
    err = np.abs(got - want)
    exact = bound == 0
    assert (err[exact] == 0).all(), f"{what}: an element that must be exact is not"
    ratio = np.where(exact, 0.0, err / np.where(exact, 1.0, bound))
    i = int(np.argmax(ratio))
    assert ratio.flat[i] <= 1.0, (f"{what}[{i}]: got {got.flat[i]!r} want {np.asarray(want).flat[i]!r}: |err| {err.flat[i]:.3e} = "
                                  f"{ratio.flat[i]:.2f} x bound {np.asarray(bound).flat[i]:.3e}")
    return float(ratio.flat[i])


def check_against(buf, ref, what, tag):
    """Device state after a step against adamw_f64's result: sumsq[0], grad_norm, p / g / m / v elementwise; canaries."""
    ss0 = float(buf.get("ss")[0])
    norm = float(buf.t["ss"][:1].sqrt().cpu().numpy()[0])                  # FusedClipAdamW.grad_norm()
    r = dict(sumsq=_ratio(np.array([ss0]), np.array([ref["sumsq"]]), np.array([ref["sumsq_bound"]]), what + " sumsq"),
             norm=_ratio(np.array([norm]), np.array([ref["norm"]]), np.array([ref["norm_bound"]]), what + " grad_norm"))
    for k in ("p", "g", "m", "v"):
        r[k] = _ratio(buf.get(k), ref[k], ref[k + "_bound"], f"{what} {k}")
    assert buf.canaries_intact(), f"{what}: a kernel wrote outside its buffers"
    w = WORST.setdefault(tag, {})
    for k, v in r.items():
        w[k] = max(w.get(k, 0.0), v)
    return r


def _report(tag):
    print(f"{tag}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.get(tag, {}).items()))


@pytest.mark.parametrize("hname", list(FC.HYPERS))
def test_clip_adamw_cross_of_hyperparameters_steps_and_gradients(hname):
    """n = 1023 (float4 body + a 3-element scalar tail): every step x gradient kind x zero_grads of this hyper-parameter set."""
    h = FC.HYPERS[hname]
    n = 1023
    for hn, step, kind, zg, seed in FC.adamw_cross_cases():
        if hn != hname:
            continue
        p, m, v = FC.adamw_state(n, seed)
        g = FC.adamw_grad(n, kind, seed)
        buf = Buffers(p, g, m, v)
        buf.step(h, step, zg)
        check_against(buf, R.adamw_f64(p, g, m, v, h, step, zg), f"{hname} step {step} g {kind} zero_grads {zg}", "clip_adamw_kernel")
    _report("clip_adamw_kernel")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", FC.SIZES)
def test_clip_adamw_sizes_and_alignment(n, offset):
    """Each size (scalar tails, one element, the grid-stride second pass from 2 097 157 elements) with the buffers 16-byte
    aligned and offset by one float (Buffers asserts data_ptr() % 16 == 4: the kernels' n4 = 0 branch)."""
    big = n > 300000
    kinds = ("above", "span") if big else FC.GRAD_KINDS
    tag = "sumsq/clip_adamw " + ("unaligned" if offset else "aligned")
    for i, kind in enumerate(kinds):
        h = FC.HYPERS["default" if i % 2 == 0 else "lr1e-2_wd0.1"]
        step, zg = (2, 1000, 10)[i % 3], (i + offset) % 2
        p, m, v = FC.adamw_state(n, n % 83 + i)
        g = FC.adamw_grad(n, kind, n % 71 + i)
        buf = Buffers(p, g, m, v, offset)
        buf.step(h, step, zg)
        check_against(buf, R.adamw_f64(p, g, m, v, h, step, zg), f"n {n} offset {offset} g {kind} step {step} zero_grads {zg}", tag)
    _report(tag)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
def test_five_steps_carried_on_the_device(offset):
    """Steps 1 .. 5 from the late state with the state carried on the device, against five steps carried in float64; the bound of
    step k propagates the first-order errors of steps < k (adamw_f64's err_in)."""
    n = 262147
    h = FC.HYPERS["lr1e-2_wd0.1"]
    p, m, v = FC.adamw_state(n, 5)
    buf = Buffers(p, FC.adamw_grad(n, "below", 0), m, v, offset)
    rp, rm, rv = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    err = None
    for step in range(1, 6):
        g = FC.adamw_grad(n, ("below", "above", "near", "span", "above")[step - 1], 40 + step)
        buf.t["g"].copy_(torch.from_numpy(g))
        buf.step(h, step, 0)
        ref = R.adamw_f64(rp, g, rm, rv, h, step, 0, err_in=err)
        check_against(buf, ref, f"carried step {step} offset {offset}", "five carried steps")
        rp, rm, rv, err = ref["p"], ref["m"], ref["v"], ref["err"]
    _report("five carried steps")


@pytest.mark.parametrize("zero_grads", [0, 1])
@pytest.mark.parametrize("badval", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("n,offset", [(1023, 0), (262147, 1)])
def test_non_finite_gradient_makes_the_step_a_no_op(n, offset, badval, zero_grads):
    """One Inf / one NaN in g: p, m, v bit-identical to before, grad_norm not finite, g cleared iff zero_grads."""
    p, m, v = FC.adamw_state(n, 9)
    g = FC.adamw_grad(n, "above", 9)
    g[n - 2] = badval
    buf = Buffers(p, g, m, v, offset)
    buf.step(FC.HYPERS["default"], 10, zero_grads)
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    for k, want in (("p", p), ("m", m), ("v", v)):
        assert np.array_equal(bits(buf.get(k)), bits(want)), k
    assert not np.isfinite(buf.t["ss"][:1].sqrt().cpu().numpy()[0])
    assert (bits(buf.get("g")) == 0).all() if zero_grads else np.array_equal(bits(buf.get("g")), bits(g))
    assert buf.canaries_intact()
    ref = R.adamw_f64(p, g, m, v, FC.HYPERS["default"], 10, zero_grads)
    assert ref["skipped"]


@pytest.mark.parametrize("zero_grads", [0, 1])
@pytest.mark.parametrize("step", [2, 1000])
def test_shadow_kernel_equals_clip_adamw_from_a_late_state(step, zero_grads, kg_real):
    """adamw_shadow_kernel on a default-dims bf16 engine's flat buffers (as optim.py calls it) with late-state moments and a
    clipped gradient: p / g / m / v bit-identical to camo_clip_adamw on copies, under the float64 bound, and the bf16 shadows it
    leaves byte-identical to those a forward rebuilds from the updated parameters."""
    from camouflage_multimodal_amd import _lib
    from test_hip_parity import make_model
    cfg = OP.full_cfg()
    h = FC.HYPERS["default"]
    m_ = make_model(cfg, 4, "bf16").train()
    eng = m_._engine
    nrs = [303, 64, 17]
    rg = torch.from_numpy(np.concatenate([OP.make_rg(k, 128, seed=30 + i) for i, k in enumerate(nrs)])).cuda()
    kg = torch.from_numpy(np.stack([kg_real] * len(nrs))).cuda()
    y, e, s = (torch.from_numpy(a) for a in OP.make_labels(len(nrs), seed=6))
    batch = eng.make_batch(rg, nrs, kg)
    gflat = eng.ensure_flat_grads(attach=False)
    eng.train_raw(batch, eng.workspace(batch), y, e, s, True, 5, eng._gtab, use_shadows=True)      # (fills the whole shadow buffer once)
    torch.cuda.synchronize()
    n = eng.flat_params.numel()
    p0 = eng.flat_params.detach().cpu().numpy().copy()
    _, m0, v0 = FC.adamw_state(n, 70 + step % 7)
    g0 = FC.adamw_grad(n, "above" if zero_grads else "span", 3 + step % 5)
    gflat.copy_(torch.from_numpy(g0))
    mt, vt = torch.from_numpy(m0).cuda(), torch.from_numpy(v0).cuda()
    ss = torch.zeros(SUMSQ_FLOATS, device="cuda")
    plain = Buffers(p0, g0, m0, v0)
    plain.step(h, step, zero_grads)
    L = _lib.lib()
    P = lambda t: C_.c_void_p(t.data_ptr())
    st = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    sh = eng.shadow_buffer()
    assert sh is not None
    _lib.check(L.camo_grad_sumsq(P(gflat), n, P(ss), st), "camo_grad_sumsq")
    with torch.no_grad():
        _lib.check(L.camo_clip_adamw_shadows(C_.byref(eng.dims), eng._ptab, P(eng.flat_params), P(gflat), P(mt), P(vt), n, P(ss), h["max_norm"],
                                             h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, zero_grads, P(sh), st), "camo_clip_adamw_shadows")
    torch.cuda.synchronize()
    got = dict(p=eng.flat_params.detach().cpu().numpy(), g=gflat.cpu().numpy(), m=mt.cpu().numpy(), v=vt.cpu().numpy())
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(plain.get(k))), f"{k}: adamw_shadow_kernel != clip_adamw_kernel"
    assert bits(ss.cpu().numpy())[0] == bits(plain.get("ss"))[0]
    check_against(plain, R.adamw_f64(p0, g0, m0, v0, h, step, zero_grads), f"engine buffers step {step} zero_grads {zero_grads}",
                  "adamw_shadow_kernel (bit-identical to clip_adamw_kernel)")
    _report("adamw_shadow_kernel (bit-identical to clip_adamw_kernel)")
    assert float(np.abs(got["p"] - p0).max()) > 0
    # the shadows it left == the shadows a forward rebuilds from those parameters (test_adamw_leaves_the_next_steps_weight_shadows)
    left = sh.clone()
    eng._shadows_version = None
    eng.train_raw(batch, eng.workspace(batch), y, e, s, True, 6, eng._gtab, use_shadows=True)
    torch.cuda.synchronize()
    assert torch.equal(left, eng._shadows)
