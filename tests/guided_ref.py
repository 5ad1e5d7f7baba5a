"""numpy restatement of include/camo_guided.h (PARITY UNPINNED: the header's text is the definition; this file shares no code with
the package).  float64 on the fp32 inputs.  Every window is summed DIRECTLY -- the clipped 2-D window of every pixel, one numpy sum
each, no running sums over the image -- so this side is the better-conditioned one; the solve is ``numpy.linalg.solve``; the apply
uses the tap integers of tests/resize_ref.py.  The kernels are held to it within the rounding of their fp32 outputs (``q_bound``,
``coef_bounds``, ``apply_bound``), the magnitudes taken from this file's own values.
"""
import numpy as np

import resize_ref as RR

U = 2.0 ** -24
LUMA = np.array([0.2989, 0.5870, 0.1140], np.float32)


def window_means(t, r):
    """t float64 [H, W, K] -> the mean of every plane over every pixel's clipped window [H, W, K]."""
    H, W = t.shape[:2]
    out = np.empty_like(t)
    for y in range(H):
        y0, y1 = max(y - r, 0), min(y + r, H - 1)
        for x in range(W):
            x0, x1 = max(x - r, 0), min(x + r, W - 1)
            out[y, x] = t[y0:y1 + 1, x0:x1 + 1].sum(axis=(0, 1)) / float((y1 - y0 + 1) * (x1 - x0 + 1))
    return out


def guided_filter(I, p, r, eps, clamp=False):
    """One image: guide I fp32 [H, W, C] (or [H, W]), p fp32 [H, W] -> dict of float64 arrays: "q" [H, W], "coef" [C + 1, H, W]
    (abar_0 .. abar_{C-1}, bbar), "mu" [H, W, C] (the window means of the guide) and "a", "b" (the per-pixel coefficients)."""
    I = np.asarray(I)
    p = np.asarray(p)
    assert I.dtype == np.float32 and p.dtype == np.float32
    if I.ndim == 2:
        I = I[:, :, None]
    H, W, C = I.shape
    I, p = I.astype(np.float64), p.astype(np.float64)
    II = I[:, :, :, None] * I[:, :, None, :]
    planes = np.concatenate([I, p[:, :, None], I * p[:, :, None], II.reshape(H, W, C * C)], axis=2)
    m = window_means(planes, r)
    mu, pbar, mIp, mII = m[:, :, :C], m[:, :, C], m[:, :, C + 1:2 * C + 1], m[:, :, 2 * C + 1:].reshape(H, W, C, C)
    sigma = mII - mu[:, :, :, None] * mu[:, :, None, :] + float(eps) * np.eye(C)
    c = mIp - mu * pbar[:, :, None]
    a = np.linalg.solve(sigma, c[:, :, :, None])[:, :, :, 0]
    b = pbar - (a * mu).sum(axis=2)
    ab = window_means(np.concatenate([a, b[:, :, None]], axis=2), r)
    abar, bbar = ab[:, :, :C], ab[:, :, C]
    q = (abar * I).sum(axis=2) + bbar
    if clamp:
        q = np.clip(q, 0.0, 1.0)
    return {"q": q, "coef": np.concatenate([abar, bbar[:, :, None]], axis=2).transpose(2, 0, 1), "mu": mu, "a": a, "b": b, "I": I}


def q_bound(ref):
    """4 * 2^-24 (sum_c |abar_c I_c| + |bbar| + 1) per pixel, from the reference's own values."""
    coef = ref["coef"]
    return 4 * U * (np.abs(coef[:-1].transpose(1, 2, 0) * ref["I"]).sum(axis=2) + np.abs(coef[-1]) + 1)


def coef_bounds(ref):
    """[C + 1, H, W]: 4 * 2^-24 (|abar_c| + 1) for the planes of abar, 4 * 2^-24 (|bbar| + |abar . mu| + 1) for bbar."""
    coef = ref["coef"]
    amu = np.abs((coef[:-1].transpose(1, 2, 0) * ref["mu"]).sum(axis=2))
    return np.concatenate([4 * U * (np.abs(coef[:-1]) + 1), (4 * U * (np.abs(coef[-1]) + amu + 1))[None]], axis=0)


def guided_apply(coef, img, clamp=False):
    """coef fp32 [C + 1, h, w], img uint8 [H, W, C] (or [H, W]) -> (q float64 [H, W], sum of the |terms| of q [H, W])."""
    coef, img = np.asarray(coef), np.asarray(img)
    assert coef.dtype == np.float32 and img.dtype == np.uint8
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    assert coef.shape[0] == C + 1
    h, w = coef.shape[1:]
    iy, wy, Ty = RR.axis_taps(0, h, H, False, RR.BILINEAR)
    ix, wx, Tx = RR.axis_taps(0, w, W, False, RR.BILINEAR)
    up = np.empty((C + 1, H, W), np.float64)
    for k in range(C + 1):
        acc = None
        for ky in range(2):                                      # the header's order: (y0, x0), (y0, x1), (y1, x0), (y1, x1)
            for kx in range(2):
                wgt = (wy[:, ky][:, None] * wx[:, kx][None, :]).astype(np.float64)
                term = wgt * coef[k][iy[:, ky]][:, ix[:, kx]].astype(np.float64)
                acc = term if acc is None else acc + term
        up[k] = acc / np.float64(Ty * Tx)
    g = img.astype(np.float64) / 255.0
    q = up[0] * g[:, :, 0]
    terms = np.abs(q)
    for c in range(1, C):
        t = up[c] * g[:, :, c]
        q, terms = q + t, terms + np.abs(t)
    q, terms = q + up[C], terms + np.abs(up[C])
    if clamp:
        q = np.clip(q, 0.0, 1.0)
    return q, terms


def apply_bound(q, terms):
    """One rounding to fp32 plus the double arithmetic's own slack: 2^-23 |ref| + 2^-45 sum |terms|."""
    return 2.0 ** -23 * np.abs(q) + 2.0 ** -45 * terms


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------
def make_guide(kind, H, W, C, seed):
    rs = np.random.RandomState(seed)
    u = rs.rand(H, W, C)
    g = {"uniform": u, "binary": np.round(u), "near": 0.5 + 1e-3 * u}[kind]
    return g.astype(np.float32)


def make_p(kind, H, W, seed):
    u = np.random.RandomState(seed + 1000).rand(H, W)
    return (u > 0.5).astype(np.float32) if kind == "binary" else u.astype(np.float32)


def disc_case():
    """The 96 x 112 case of DESIGN.md 10i: (image fp32 [H, W, 3], painted mask fp32 [H, W], the disc bool [H, W])."""
    rs = np.random.RandomState(0)
    H, W = 96, 112
    yy, xx = np.mgrid[:H, :W]
    disc = (yy - 50) ** 2 + (xx - 55) ** 2 < 30 ** 2
    img = np.where(disc[:, :, None], [0.55, 0.50, 0.42], [0.45, 0.50, 0.50]) + rs.normal(0, 0.03, (H, W, 3))
    img = np.clip(img, 0, 1).astype(np.float32)
    p = np.zeros((H, W), np.float32)
    for y in range(0, H, 12):
        for x in range(0, W, 12):
            p[y:y + 12, x:x + 12] = 0.9 if disc[y:y + 12, x:x + 12].mean() > 0.5 else 0.1
    return img, p, disc


def grey(img):
    return (img @ LUMA).astype(np.float32)


def iou(mask, truth):
    return float((mask & truth).sum()) / float((mask | truth).sum())
