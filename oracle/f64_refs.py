"""float64 references of the two pieces of arithmetic that end every training step -- the four-term loss with its gradient
(csrc/misc.hip, loss_sample) and clip + AdamW (sumsq_kernel / clip_adamw_kernel / adamw_shadow_kernel) -- each with a
per-element first-order error bound for a float32 implementation.  TEST INFRASTRUCTURE (see oracle/__init__.py).

Plain numpy float64, no float32 intermediates: inputs are the float32 values the kernels get, widened.

Notation: u = 2^-24 (the unit roundoff of float32: one correctly rounded operation has relative error <= u), ulp = 2 u (one
unit in the last place, relative to the result, at worst), TINY = 2^-126 (the smallest normal float32: hardware exp / rcp / log
flush what is below it, so every transcendental's result carries TINY as an absolute allowance).

THE BOUND of an element is  2 x (first-order propagation of one rounding per float32 operation) + one ulp of the result.
The first-order sum is written next to each formula below ("d" + name = absolute error of that intermediate).

Allowances, each stated once:
  * + - * / sqrt fma in float32                       u relative (IEEE; hipcc rounds / and sqrt correctly by default)
  * the subtraction 1 - pt                            u absolute (issue: the cancellation enters as an absolute u)
  * library expf / logf / log1pf / division           2 ulp of the result (ROCm's device-library documentation gives ~1 ulp)
  * FAST __expf(x)                                    (2 + |x| log2(e)) ulp: v_exp_f32 is ~1 ulp of 2^t, and t = x * log2(e) was
                                                      rounded before it -- |t| u absolute in the exponent = |x| log2(e) u relative
  * FAST __logf(x)                                    2 ulp of the result + u absolute (its argument's rounding, at x ~ 1)
  * FAST __frcp_rn                                    1 ulp
  * sum of squares over n elements                    (L + 16) u relative, L = ceil(n / 65 536) fused multiply-adds per lane
                                                      (256 blocks x 256 lanes), 16 = the additions of the reduction tree
                                                      (6 + 2 in sumsq_kernel's block, 6 + 2 over the 256 partials)
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
ULP = 2.0 ** -23
TINY = 2.0 ** -126
LOG2E = 1.4426950408889634
LOSS_W = (3.0, 1.0, 0.5, 0.3)          # train_multimodal.py:257,260,263,266

LOSS_MUTATIONS = ("alpha_swapped", "alpha_all_ge1", "gamma2", "focal_grad_no_ce_term", "bce_no_max", "dpre_no_sigmoid_slope",
                  "mse_grad_weight_03", "pred_last_max")
ADAMW_MUTATIONS = ("no_decay", "l2_decay", "decay_after", "eps_inside_sqrt", "bc2_no_root", "step_minus_1", "no_clamp", "m_unclipped")


def sigmoid_f64(x):
    x = np.asarray(x, np.float64)
    ex = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + ex), ex / (1.0 + ex))


def _final(first_order, result):
    return 2.0 * first_order + ULP * np.abs(result) + TINY


def _softmax_parts(o, yy, fast):
    """Per row of o [B, C]: log-sum-exp pieces as loss_sample computes them, with first-order errors.
    -> ce [B], dce, pk [B, C], dpk."""
    B, C = o.shape
    idx = np.arange(B)
    mx = o.max(1)
    d = o - mx[:, None]                                      # float32 subtraction:                dd = u |d|
    dd = U * np.abs(d)
    ek = np.exp(d)                                           # exp: argument error + the function's own
    ulps = (2.0 + np.abs(d) * LOG2E) if fast else 2.0
    dek = ek * dd + ek * ulps * ULP + TINY
    z = ek.sum(1)                                            # C - 1 sequential additions of positive terms
    dz = dek.sum(1) + (C - 1) * U * z
    lgz = np.log(z)                                          # log: 2 ulp (+ u absolute when FAST) + argument error
    dlg = dz / z + 2.0 * ULP * np.abs(lgz) + (U if fast else 0.0) + TINY
    ce = -(d[idx, yy] - lgz)                                 # one subtraction
    dce = dd[idx, yy] + dlg + U * np.abs(ce)
    if fast:                                                 # pk = ex(.) * rcp(z)
        iz = 1.0 / z
        diz = iz * (dz / z + ULP) + TINY
        pk = ek * iz[:, None]
        dpk = dek * iz[:, None] + ek * diz[:, None] + U * pk + TINY
    else:                                                    # pk = expf(.) / z
        pk = ek / z[:, None]
        dpk = dek / z[:, None] + pk * (dz / z)[:, None] + 2.0 * ULP * pk + TINY
    return ce, dce, pk, dpk


def loss_f64(outs, y, e, s, C, fast=False, mutation=None):
    """The per-sample loss 3 focal(mask, y) + CE(instance, y) + .5 BCEWithLogits(edge, e) + .3 MSE(score, s) of
    train_multimodal.py:29-57, 256-268 (as losses.py and FO.sample_loss restate it): focal alpha .75 for class 1 and .25 otherwise,
    gamma 3, from a log-sum-exp; the score column of ``outs`` is post-sigmoid.

    outs [B, 2C+2] float32, y int [B] in [0, C), e / s float32 [B].  -> dict:
      terms [B, 4] (weighted), d_outs [B, 2C+2], d_pre (d_outs with the score column times s (1 - s): the gradient w.r.t. the
      score head's pre-sigmoid value), pred [B] (the first maximum of the mask logits),
      terms_bound, d_outs_bound, d_pre_bound: the per-element bounds of the module docstring, for the library-math variant of
      loss_sample or (``fast``) its hardware-intrinsic variant.
    ``mutation``: one of LOSS_MUTATIONS -- a deliberately wrong copy, for the tests that show the bounds have teeth."""
    assert mutation is None or mutation in LOSS_MUTATIONS, mutation
    o = np.asarray(outs, np.float64)
    B, W = o.shape
    assert W == 2 * C + 2
    yy = np.asarray(y, np.int64)
    assert ((yy >= 0) & (yy < C)).all()
    ev = np.asarray(e, np.float64); sv = np.asarray(s, np.float64)
    idx = np.arange(B)
    terms = np.zeros((B, 4)); dterms = np.zeros((B, 4))
    g = np.zeros((B, W)); dg = np.zeros((B, W))
    onehot = np.zeros((B, C)); onehot[idx, yy] = 1.0

    # ---- focal on the mask logits: l = 3 at om^3 ce, om = 1 - pt;  d l / d logit_k = 3 at (-3 om^2 ce pt - om^3) (delta_ky - p_k)
    om_ = o[:, :C]
    ce, dce, pk, dpk = _softmax_parts(om_, yy, fast)
    pt, dpt = pk[idx, yy], dpk[idx, yy]
    if mutation == "alpha_swapped":
        at = np.where(yy == 1, 0.25, 0.75)
    elif mutation == "alpha_all_ge1":
        at = np.where(yy >= 1, 0.75, 0.25)
    else:
        at = np.where(yy == 1, 0.75, 0.25)
    om = 1.0 - pt                                            # dom = dpt + u (absolute)
    dom = dpt + U
    if mutation == "gamma2":
        terms[:, 0] = 3.0 * at * om ** 2 * ce
        dl = at * (-2.0 * om * ce * pt - om ** 2)
    else:
        terms[:, 0] = 3.0 * at * om ** 3 * ce                # four multiplications
        dl = at * (-3.0 * om ** 2 * ce * pt - om ** 3)
    if mutation == "focal_grad_no_ce_term":
        dl = at * (-om ** 3)
    dterms[:, 0] = 3.0 * at * (3.0 * om ** 2 * dom * ce + om ** 3 * dce) + 5.0 * U * np.abs(terms[:, 0])
    a_ = 3.0 * om ** 2 * ce * pt; b_ = om ** 3               # dl = at (-a - b): four + two multiplications, a subtraction, times at
    da = 3.0 * (2.0 * om * dom * ce * pt + om ** 2 * dce * pt + om ** 2 * ce * dpt) + 4.0 * U * a_
    db = 3.0 * om ** 2 * dom + 2.0 * U * b_
    ddl = at * (da + db) + 2.0 * U * np.abs(dl)
    q = onehot - pk                                          # one subtraction
    dq = dpk + U * np.abs(q)
    g[:, :C] = 3.0 * dl[:, None] * q                         # two multiplications
    dg[:, :C] = 3.0 * (ddl[:, None] * np.abs(q) + np.abs(dl)[:, None] * dq) + 2.0 * U * np.abs(g[:, :C])
    mx = om_.max(1)
    if mutation == "pred_last_max":
        pred = C - 1 - np.argmax(om_[:, ::-1] == mx[:, None], axis=1)
    else:
        pred = np.argmax(om_ == mx[:, None], axis=1)         # the first maximum

    # ---- cross entropy on the instance logits: l = ce;  d l / d logit_k = p_k - delta_ky
    ce1, dce1, pk1, dpk1 = _softmax_parts(o[:, C:2 * C], yy, fast)
    terms[:, 1] = ce1; dterms[:, 1] = dce1
    g[:, C:2 * C] = pk1 - onehot
    dg[:, C:2 * C] = dpk1 + U * np.abs(g[:, C:2 * C])

    # ---- BCE with logits on the edge logit: l = .5 (max(x, 0) - x t + log1p(exp(-|x|)));  d l / d x = .5 (sigmoid(x) - t)
    x = o[:, 2 * C]; t = ev
    ea = np.exp(-np.abs(x))
    dea = ea * ((2.0 + np.abs(x) * LOG2E) if fast else 2.0) * ULP + TINY
    L = np.log1p(ea)
    if fast:                                                 # __logf(1 + __expf(.)): the addition rounds, then the log
        w = 1.0 + ea
        dL = (dea + U * w) / w + 2.0 * ULP * L + U + TINY
    else:                                                    # log1pf(expf(.))
        dL = dea / (1.0 + ea) + 2.0 * ULP * L + TINY
    mxx = 0.0 if mutation == "bce_no_max" else np.maximum(x, 0.0)
    inner = mxx - x * t + L                                  # a product, two additions
    terms[:, 2] = 0.5 * inner
    dterms[:, 2] = 0.5 * (U * np.abs(x * t) + U * np.abs(mxx - x * t) + dL + U * np.abs(inner))
    sg = sigmoid_f64(x)                                      # 1 / (1 + exp(-x)): d sg = sg (1 - sg) (relative error of the exp) + add + divide
    dsg = sg * (1.0 - sg) * ((2.0 + np.abs(x) * LOG2E) if fast else 2.0) * ULP + U * sg + (ULP if fast else 2.0 * ULP) * sg + TINY
    g[:, 2 * C] = 0.5 * (sg - t)
    dg[:, 2 * C] = 0.5 * (dsg + U * np.abs(sg - t))

    # ---- MSE on the post-sigmoid score: l = .3 (x - t)^2;  d l / d x = .6 (x - t)
    x = o[:, 2 * C + 1]; t = sv
    df = x - t                                               # one subtraction; .3f and .6f are themselves rounded (u each)
    ddf = U * np.abs(df)
    terms[:, 3] = 0.3 * df * df
    dterms[:, 3] = 0.6 * np.abs(df) * ddf + 3.0 * U * terms[:, 3]
    wg = 0.3 if mutation == "mse_grad_weight_03" else 0.6
    g[:, 2 * C + 1] = wg * df
    dg[:, 2 * C + 1] = 0.6 * ddf + 2.0 * U * np.abs(g[:, 2 * C + 1])

    # ---- d_pre: the score column times the sigmoid's slope sc (1 - sc): a subtraction and two multiplications
    d_pre = g.copy(); dd_pre = dg.copy()
    sc = o[:, W - 1]
    slope = 1.0 if mutation == "dpre_no_sigmoid_slope" else sc * (1.0 - sc)
    d_pre[:, W - 1] = g[:, W - 1] * slope
    dd_pre[:, W - 1] = dg[:, W - 1] * np.abs(sc * (1.0 - sc)) + 3.0 * U * np.abs(d_pre[:, W - 1])
    return dict(terms=terms, d_outs=g, d_pre=d_pre, pred=pred.astype(np.int64),
                terms_bound=_final(dterms, terms), d_outs_bound=_final(dg, g), d_pre_bound=_final(dd_pre, d_pre))


# ------------------------------------------------------------------------------------------------------------------ clip + AdamW
def sumsq_rel_error(n):
    """First-order relative error of sumsq_kernel's float32 sum of squares over n elements (module docstring)."""
    return (int(np.ceil(n / 65536.0)) + 16) * U


def adamw_f64(p, g, m, v, hyper, step, zero_grads, err_in=None, mutation=None):
    """torch.nn.utils.clip_grad_norm_(max_norm) then torch.optim.AdamW.step() at 1-based ``step``, as clip_adamw_kernel restates them:
        norm = sqrt(sum g^2);  coef = min(1, max_norm / (norm + 1e-6));  g <- g coef
        p <- p (1 - lr wd)                                   (decoupled decay first)
        m <- b1 m + (1 - b1) g;   v <- b2 v + (1 - b2) g^2
        denom = sqrt(v) / sqrt(bc2) + eps;   p <- p - lr / bc1 * m / denom,      bc_i = 1 - b_i^step
    A norm that is not finite makes the step a no-op (p, m, v stay); g is then cleared only if ``zero_grads``, as it is after a
    normal step (otherwise the clipped gradients stay in it).

    p, g, m, v: float32 arrays (widened here); hyper: dict(lr, wd, b1, b2, eps, max_norm), rounded to float32 first as the C ABI
    does.  -> dict(p, g, m, v, sumsq, norm, skipped, *_bound per element, sumsq_bound, norm_bound, err=(dp, dm, dv)).
    ``err_in`` = the ``err`` of the previous step when the state was carried on the device (its first-order errors propagate).
    ``mutation``: one of ADAMW_MUTATIONS."""
    assert mutation is None or mutation in ADAMW_MUTATIONS, mutation
    f = lambda k: float(np.float32(hyper[k]))
    lr, wd, b1, b2, eps, max_norm = f("lr"), f("wd"), f("b1"), f("b2"), f("eps"), f("max_norm")
    p = np.asarray(p, np.float64); g = np.asarray(g, np.float64); m = np.asarray(m, np.float64); v = np.asarray(v, np.float64)
    n = p.size
    dp0, dm0, dv0 = err_in if err_in is not None else (0.0, 0.0, 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        sumsq = float((g * g).sum())
    norm = float(np.sqrt(sumsq)) if sumsq >= 0 else float("nan")
    es = sumsq_rel_error(n)
    out = dict(sumsq=sumsq, norm=norm, sumsq_bound=2.0 * es * sumsq + ULP * sumsq + TINY,
               norm_bound=2.0 * (es / 2.0 + U) * norm + ULP * norm + TINY)     # sqrt halves the relative error and rounds once
    if not np.isfinite(sumsq):
        gz = np.zeros_like(g) if zero_grads else g.copy()
        z = np.zeros_like(p)
        out.update(p=p.copy(), g=gz, m=m.copy(), v=v.copy(), skipped=True, p_bound=z, g_bound=z, m_bound=z, v_bound=z, err=(dp0, dm0, dv0))
        return out
    # coef: sqrt (es / 2 + u), + 1e-6 (u), the division (u), 1e-6f's own rounding (u); min(1, .) is 1-Lipschitz
    coef = max_norm / (norm + 1e-6)
    if mutation != "no_clamp":
        coef = min(1.0, coef)
    rcoef = es / 2.0 + 4.0 * U
    gc = g * coef                                            # one multiplication
    dgc = np.abs(gc) * (rcoef + U)
    step_b = step - 1 if mutation == "step_minus_1" else step
    bc1 = 1.0 - b1 ** step_b; bc2 = 1.0 - b2 ** step_b
    decay = 1.0 if mutation == "no_decay" else 1.0 - lr * wd  # a product and a subtraction in float32: 2 u
    gm = g if mutation == "m_unclipped" else gc
    gl = gc + wd * p if mutation == "l2_decay" else gc
    if mutation == "l2_decay":
        decay, gm = 1.0, gl
    p1 = p * decay
    dp1 = dp0 * decay + np.abs(p) * 2.0 * U + U * np.abs(p1)
    m2 = m * b1 + gm * (1.0 - b1)                            # two products and an addition, 1 - b1 rounded (u)
    dm2 = dm0 * b1 + U * np.abs(m * b1) + dgc * (1.0 - b1) + 2.0 * U * np.abs(gc) * (1.0 - b1) + U * np.abs(m2)
    v2 = v * b2 + gl * gl * (1.0 - b2)                       # three products and an addition, 1 - b2 rounded (u)
    dv2 = dv0 * b2 + U * np.abs(v * b2) + 2.0 * np.abs(gc) * dgc * (1.0 - b2) + 3.0 * U * gc * gc * (1.0 - b2) + U * np.abs(v2)
    if mutation == "eps_inside_sqrt":
        den = np.sqrt(v2 / bc2 + eps)
    elif mutation == "bc2_no_root":
        den = np.sqrt(v2) / bc2 + eps
    else:
        den = np.sqrt(v2) / np.sqrt(bc2) + eps
    sq = np.sqrt(v2)                                         # d sqrt = dv / (2 sqrt v) + u sqrt v
    with np.errstate(divide="ignore", invalid="ignore"):
        dsq = np.where(v2 > 0, dv2 / (2.0 * np.where(v2 > 0, sq, 1.0)), 0.0) + U * sq
    isb2 = 1.0 / np.sqrt(bc2) if bc2 > 0 else float("inf")   # rounded to float32 by the host (u), a product (u), an addition (u)
    dden = dsq * isb2 + 2.0 * U * sq * isb2 + U * np.abs(den)
    r = m2 / den                                             # one division
    dr = dm2 / den + np.abs(m2) * dden / (den * den) + U * np.abs(r)
    stp = lr / bc1 if bc1 != 0 else float("inf")             # lr * float32(1 / bc1): 2 u
    upd = stp * r                                            # one more product
    dupd = stp * dr + 3.0 * U * np.abs(upd)
    p2 = p1 - upd                                            # one subtraction
    if mutation == "decay_after":
        p2 = (p - upd) * (1.0 - lr * wd)
    dp2 = dp1 + dupd + U * np.abs(p2)
    g_out = np.zeros_like(g) if zero_grads else gc
    out.update(p=p2, g=g_out, m=m2, v=v2, skipped=False, coef=coef,
               p_bound=_final(dp2, p2), m_bound=_final(dm2, m2), v_bound=_final(dv2, v2),
               g_bound=np.zeros_like(g) if zero_grads else _final(dgc, gc), err=(dp2, dm2, dv2))
    return out
