"""camo_loss (csrc/misc.hip: loss_kernel, the library-math instantiation of loss_sample) against the float64 reference
oracle/f64_refs.loss_f64, on its own -- no model in front of it.  Needs an MI355X.

Inputs: tests/f64_cases.loss_grid -- C in {1, 2, 3, 8, 9, 64}, B in {1, 63, 64, 65, 1000} (64-thread blocks), every label of every
C, logit rows of magnitude 0 ... 100 with the true class largest / smallest / tied, all logits equal, a logit gap of 120 (pt
underflows, CE stays finite), edge logits 0 ... +-100 x labels {0, 1, .3}, scores {0, 1e-7, .5, 1 - 1e-7, 1} x labels.
tests/test_f64_refs.py shows on the CPU that each of eight plausible errors exceeds the bound 10 x somewhere on this grid.

Every element of terms, d_outs and d_pre must sit under loss_f64's per-element bound (2 x the first-order propagation of one
rounding per float32 operation + 1 ulp; the allowances and their sources are listed once, in oracle/f64_refs.py's docstring);
pred must be exact.  Nothing is exempted and nothing is tuned: a ratio error / bound above 1 is a finding.

Largest observed error / bound over the whole grid (MI355X, library variant):  terms 0.27, d_outs 0.37, d_pre 0.37
(C = 8; per class count the test prints its own).
"""
import ctypes as C_

import numpy as np
import pytest
import torch

import f64_cases as FC
from oracle import f64_refs as R

pytestmark = pytest.mark.gpu

PAD = 67                      # canary elements on each side of every output buffer
CANARY_F = -12345.678
CANARY_I = -77


def _guarded(n, dtype):
    buf = torch.full((n + 2 * PAD,), CANARY_I if dtype is torch.int32 else CANARY_F, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _canaries_intact(buf, n):
    want = CANARY_I if buf.dtype is torch.int32 else np.float32(CANARY_F)
    b = buf.cpu().numpy()
    return (b[:PAD] == want).all() and (b[PAD + n:] == want).all()


def raw_loss(outs, y, e, s, C, want=("d_outs", "d_pre", "pred")):
    """camo_loss through the raw ABI on guarded buffers -> dict of numpy arrays (None for an output passed as NULL)."""
    from camouflage_multimodal_amd import _lib
    B, W = outs.shape
    assert W == 2 * C + 2
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dt).contiguous()
    o, yy, ee, ss = to(outs, torch.float32), to(y, torch.int64), to(e, torch.float32), to(s, torch.float32)
    tb, terms = _guarded(4 * B, torch.float32)
    db, d_outs = _guarded(B * W, torch.float32)
    pb, d_pre = _guarded(B * W, torch.float32)
    rb, pred = _guarded(B, torch.int32)
    P = lambda t, on=True: C_.c_void_p(t.data_ptr()) if on else C_.c_void_p(0)
    rc = _lib.lib().camo_loss(P(o), P(yy), P(ee), P(ss), B, C, P(terms), P(d_outs, "d_outs" in want), P(d_pre, "d_pre" in want),
                              P(pred, "pred" in want), C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "camo_loss")
    torch.cuda.synchronize()
    assert _canaries_intact(tb, 4 * B) and _canaries_intact(db, B * W) and _canaries_intact(pb, B * W) and _canaries_intact(rb, B), \
        f"camo_loss wrote outside an output buffer (B {B}, C {C})"
    # an output passed as NULL: its (unused) buffer must be untouched as well
    for name, t in (("d_outs", d_outs), ("d_pre", d_pre)):
        if name not in want:
            assert (t == np.float32(CANARY_F)).all(), name
    if "pred" not in want:
        assert (pred == CANARY_I).all()
    n = lambda t: t.cpu().numpy().copy()
    return dict(terms=n(terms).reshape(B, 4), d_outs=n(d_outs).reshape(B, W) if "d_outs" in want else None,
                d_pre=n(d_pre).reshape(B, W) if "d_pre" in want else None, pred=n(pred) if "pred" in want else None)


def worst_ratio(got, ref, key, rows=None, what=""):
    """max |got - ref| / bound over the elements (of ``rows``); asserts it is <= 1 and everything is finite."""
    g = np.asarray(got, np.float64); want = ref[key]; bound = ref[key + "_bound"]
    if rows is not None:
        g, want, bound = g[rows], want[rows], bound[rows]
    assert np.isfinite(g).all(), f"{what} {key}: non-finite value"
    ratio = np.abs(g - want) / bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio[i] <= 1.0, f"{what} {key}{i}: got {g[i]!r} want {want[i]!r}: |err| {abs(g[i] - want[i]):.3e} = {ratio[i]:.2f} x bound {bound[i]:.3e}"
    return float(ratio[i])


@pytest.mark.parametrize("C", FC.LOSS_CLASSES)
def test_camo_loss_matches_float64_reference_over_the_grid(C):
    from camouflage_multimodal_amd.losses import multitask_loss
    outs, y, e, s, _ = FC.loss_grid(C)
    worst = dict(terms=0.0, d_outs=0.0, d_pre=0.0)
    seen = np.zeros(len(y), bool)
    for B, rows in FC.loss_calls(C):
        o, yy, ee, ss = outs[rows], y[rows], e[rows], s[rows]
        ref = R.loss_f64(o, yy, ee, ss, C)
        got = raw_loss(o, yy, ee, ss, C)
        what = f"C {C} B {B}"
        for k in worst:
            worst[k] = max(worst[k], worst_ratio(got[k], ref, k, what=what))
        assert np.array_equal(got["pred"], ref["pred"]), what
        seen[rows] = True
        # the public wrapper: the same numbers (it passes d_outs XOR d_pre)
        ot = torch.from_numpy(o).cuda()
        for pre in (False, True):
            t, d, p = multitask_loss(ot, torch.from_numpy(yy), torch.from_numpy(ee), torch.from_numpy(ss), C, pre_activation=pre)
            assert np.array_equal(t.cpu().numpy(), got["terms"]) and np.array_equal(p.cpu().numpy(), got["pred"])
            assert np.array_equal(d.cpu().numpy(), got["d_pre" if pre else "d_outs"])
    assert seen.all()
    print(f"camo_loss C = {C}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("C", [1, 3, 64])
def test_camo_loss_null_outputs_leave_the_others_bit_identical(C):
    outs, y, e, s, _ = FC.loss_grid(C)
    rows = (5 + np.arange(65)) % len(y)
    o, yy, ee, ss = outs[rows], y[rows], e[rows], s[rows]
    full = raw_loss(o, yy, ee, ss, C)
    for want in ((), ("d_outs",), ("d_pre",), ("pred",), ("d_outs", "pred"), ("d_pre", "pred"), ("d_outs", "d_pre")):
        got = raw_loss(o, yy, ee, ss, C, want=want)
        assert np.array_equal(got["terms"], full["terms"]), want
        for k in want:
            assert np.array_equal(got[k], full[k]), (want, k)


@pytest.mark.parametrize("C", [1, 2, 9, 64])
def test_camo_loss_out_of_range_label_poisons_its_own_focal_term_only(C):
    """Through the raw ABI (the wrappers refuse such labels on the host): label -1 and label C give NaN in that sample's focal
    term and mask-logit gradients and nothing else -- its other three terms and gradients are those of label 0, which the kernel
    substitutes instead of indexing out of bounds -- and the neighbouring samples are untouched."""
    outs, y, e, s, _ = FC.loss_grid(C)
    B = 65
    rows = (11 + np.arange(B)) % len(y)
    o, yy, ee, ss = outs[rows], y[rows].copy(), e[rows], s[rows]
    bad = np.array([0, 7, 63, 64])
    yy_bad = yy.copy(); yy_bad[bad] = [-1, C, C, -1]
    yy_ref = yy.copy(); yy_ref[bad] = 0
    ref = R.loss_f64(o, yy_ref, ee, ss, C)
    got = raw_loss(o, yy_bad, ee, ss, C)
    good = np.setdiff1d(np.arange(B), bad)
    for k in ("terms", "d_outs", "d_pre"):
        worst_ratio(got[k], ref, k, rows=good, what=f"neighbours, C {C}")
    assert np.array_equal(got["pred"], ref["pred"])
    assert np.isnan(got["terms"][bad, 0]).all()
    assert np.isnan(got["d_outs"][bad, :C]).all() and np.isnan(got["d_pre"][bad, :C]).all()
    sub = {k: ref[k][bad][:, 1:] for k in ("terms", "terms_bound")}
    worst_ratio(got["terms"][bad][:, 1:], sub, "terms", what=f"bad-label samples' other terms, C {C}")
    for k in ("d_outs", "d_pre"):
        sub = {k: ref[k][bad][:, C:], k + "_bound": ref[k + "_bound"][bad][:, C:]}
        worst_ratio(got[k][bad][:, C:], sub, k, what=f"bad-label samples' other gradients, C {C}")


def test_camo_loss_refuses_what_it_cannot_take():
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    t = torch.zeros(300, device="cuda"); yl = torch.zeros(4, dtype=torch.int64, device="cuda")
    P = lambda x: C_.c_void_p(x.data_ptr())
    for B, C in ((0, 2), (1, 0), (1, 65)):
        assert L.camo_loss(P(t), P(yl), P(t), P(t), B, C, P(t), None, None, None, None) == -1
    assert L.camo_loss(P(t), P(yl), P(t), P(t), 1, 2, None, None, None, None, None) == -1
