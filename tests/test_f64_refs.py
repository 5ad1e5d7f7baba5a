"""oracle/f64_refs.py pinned on the CPU: the float64 loss reference against central differences of its own terms and against
FO.sample_loss, the float64 AdamW reference against torch.optim.AdamW + clip_grad_norm_, and TEETH -- every listed mutation of
either reference exceeds the per-element bound by at least 10 x somewhere on the inputs the GPU tests run the kernels on
(tests/f64_cases.py), so an error of that kind in a kernel cannot pass tests/test_hip_loss.py / tests/test_hip_optimizer.py."""
import numpy as np
import pytest
import torch

import f64_cases as FC
from oracle import f64_refs as R
from oracle import fusion_oracle as FO

TEETH = 10.0


@pytest.mark.parametrize("C", FC.LOSS_CLASSES)
def test_loss_f64_gradient_is_the_central_difference_of_its_terms(C):
    outs, y, e, s, _ = FC.loss_grid(C)
    ref = R.loss_f64(outs, y, e, s, C)
    x0 = outs.astype(np.float64)
    total = lambda x: R.loss_f64(x, y, e, s, C)["terms"].sum(1)
    worst = 0.0
    for k in range(2 * C + 2):
        h = 1e-5 * np.maximum(1.0, np.abs(x0[:, k]))
        xp, xm = x0.copy(), x0.copy()
        xp[:, k] += h; xm[:, k] -= h
        fd = (total(xp) - total(xm)) / (2 * h)
        err = np.abs(fd - ref["d_outs"][:, k])
        # truncation h^2 f''' / 6 (|f'''| of the focal term reaches ~10) + cancellation 1e-16 |f| / h with |f| up to ~600
        tol = 2e-8 + 1e-6 * np.abs(ref["d_outs"][:, k])
        assert (err <= tol).all(), (C, k, int(np.argmax(err - tol)), float(err.max()))
        worst = max(worst, float(err.max()))
    # d_pre: the score column times s (1 - s), everything else as d_outs
    sc = x0[:, -1]
    assert np.array_equal(ref["d_pre"][:, :-1], ref["d_outs"][:, :-1])
    assert np.allclose(ref["d_pre"][:, -1], ref["d_outs"][:, -1] * sc * (1 - sc), rtol=1e-15, atol=0)
    assert np.isfinite(ref["terms"]).all() and np.isfinite(ref["d_outs"]).all()
    assert (ref["pred"] == np.argmax(outs[:, :C], axis=1)).all()


@pytest.mark.parametrize("C", FC.LOSS_CLASSES)
def test_loss_f64_agrees_with_the_float32_oracle_at_initialisation_scale(C):
    outs, y, e, s, init = FC.loss_grid(C)
    assert init.sum() >= 3
    ref = R.loss_f64(outs, y, e, s, C)
    tol = lambda want: 16 * R.U * (1.0 + np.abs(want))        # a dozen float32 operations on O(1) intermediates
    for i in np.nonzero(init)[0]:
        ob = dict(mask=outs[i, :C], instance=outs[i, C:2 * C], edge=outs[i, 2 * C:2 * C + 1], score=outs[i, 2 * C + 1:])
        _, terms, d = FO.sample_loss(ob, int(y[i]), float(e[i]), float(s[i]))
        got = np.concatenate([np.ravel(d[k]) for k in ("mask", "instance", "edge", "score")]).astype(np.float64)
        assert (np.abs(terms - ref["terms"][i]) <= tol(ref["terms"][i])).all(), (C, i, terms, ref["terms"][i])
        assert (np.abs(got - ref["d_outs"][i]) <= tol(ref["d_outs"][i])).all(), (C, i)


@pytest.mark.parametrize("fast", [False, True], ids=["library", "fast"])
@pytest.mark.parametrize("mutation", R.LOSS_MUTATIONS)
def test_loss_bounds_have_teeth(mutation, fast):
    """Each wrong loss exceeds the bound of the variant by >= 10 x somewhere on the grid (pred: differs somewhere)."""
    worst = 0.0
    for C in FC.LOSS_CLASSES:
        outs, y, e, s, _ = FC.loss_grid(C)
        ref = R.loss_f64(outs, y, e, s, C, fast=fast)
        bad = R.loss_f64(outs, y, e, s, C, fast=fast, mutation=mutation)
        if mutation == "pred_last_max":
            worst = max(worst, float("inf") if (bad["pred"] != ref["pred"]).any() else 0.0)
            continue
        for k in ("terms", "d_outs", "d_pre"):
            worst = max(worst, float((np.abs(bad[k] - ref[k]) / ref[k + "_bound"]).max()))
    assert worst >= TEETH, (mutation, worst)


# ------------------------------------------------------------------------------------------------------------------ clip + AdamW
@pytest.mark.parametrize("hname", list(FC.HYPERS))
@pytest.mark.parametrize("kind", ["below", "above", "span"])
def test_adamw_f64_is_torch_adamw_after_clip_grad_norm(hname, kind):
    h = FC.HYPERS[hname]
    n = 1023
    p0, m0, v0 = FC.adamw_state(n, 1)
    prm = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.AdamW([prm], lr=float(np.float32(h["lr"])), weight_decay=float(np.float32(h["wd"])),
                            betas=(float(np.float32(h["b1"])), float(np.float32(h["b2"]))), eps=float(np.float32(h["eps"])))
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = FC.adamw_grad(n, kind, 10 * step)
        prm.grad = torch.from_numpy(g.astype(np.float64))
        tn = torch.nn.utils.clip_grad_norm_([prm], max_norm=h["max_norm"])
        want_g = prm.grad.numpy().copy()
        opt.step()
        # (float32 state arrays would round between steps: the reference is stepped on its own float64 state)
        ref = _f64_step(p, g, m, v, h, step)
        assert abs(ref["norm"] - float(tn)) <= 1e-12 * float(tn)
        assert np.allclose(ref["g"], want_g, rtol=1e-12, atol=0)
        st = opt.state[prm]
        assert np.allclose(ref["m"], st["exp_avg"].numpy(), rtol=1e-11, atol=1e-300)
        assert np.allclose(ref["v"], st["exp_avg_sq"].numpy(), rtol=1e-11, atol=1e-300)
        assert np.allclose(ref["p"], prm.detach().numpy(), rtol=1e-11, atol=1e-15), (step, np.abs(ref["p"] - prm.detach().numpy()).max())
        p, m, v = ref["p"], ref["m"], ref["v"]


def _f64_step(p, g, m, v, h, step):
    """adamw_f64 on float64 state (its asarray(float64) keeps the carried values exact)."""
    return R.adamw_f64(p, g, m, v, h, step, zero_grads=False)


def test_adamw_f64_skips_a_step_whose_norm_is_not_finite():
    n = 37
    p, m, v = FC.adamw_state(n, 2)
    for badval in (np.inf, np.nan):
        for zg in (0, 1):
            g = FC.adamw_grad(n, "below", 3); g[5] = badval
            ref = R.adamw_f64(p, g, m, v, FC.HYPERS["default"], 7, zg)
            assert ref["skipped"] and not np.isfinite(ref["norm"])
            assert np.array_equal(ref["p"], p) and np.array_equal(ref["m"], m) and np.array_equal(ref["v"], v)
            assert (ref["g"] == 0).all() if zg else np.array_equal(ref["g"], g.astype(np.float64), equal_nan=True)


@pytest.mark.parametrize("mutation", R.ADAMW_MUTATIONS)
def test_adamw_bounds_have_teeth(mutation):
    """Each wrong optimizer exceeds the per-element bound by >= 10 x somewhere on the n = 1023 cross of hyper-parameters, steps,
    gradient kinds and zero_grads that tests/test_hip_optimizer.py runs."""
    n = 1023
    worst = 0.0
    for hname, step, kind, zg, seed in FC.adamw_cross_cases():
        if mutation == "step_minus_1" and step == 1:
            continue                                          # (bc = 0: the mutant divides by zero; the other steps show it)
        h = FC.HYPERS[hname]
        p, m, v = FC.adamw_state(n, seed)
        g = FC.adamw_grad(n, kind, seed)
        ref = R.adamw_f64(p, g, m, v, h, step, zg)
        bad = R.adamw_f64(p, g, m, v, h, step, zg, mutation=mutation)
        for k in ("p", "g", "m", "v"):
            b = ref[k + "_bound"]
            err = np.abs(bad[k] - ref[k])
            ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
            worst = max(worst, float(ratio.max()))
        if worst >= TEETH:
            return
    assert worst >= TEETH, (mutation, worst)


def test_span_gradient_stays_in_the_normal_range_after_clipping():
    for n in FC.SIZES[1:]:
        g = FC.adamw_grad(n, "span", n % 89).astype(np.float64)
        coef = min(1.0, 1.0 / (np.sqrt((g * g).sum()) + 1e-6))
        assert np.abs(g).min() * coef >= 1e-15 and np.abs(g).max() == 1e3 and np.abs(g).min() <= 1e-11, (n, np.abs(g).min() * coef)
