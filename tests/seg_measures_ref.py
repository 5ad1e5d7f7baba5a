"""numpy restatement of include/camo_seg_measures.h FROM THE PIXEL ARRAYS: the checker of the histogram kernels, of the host ratios in
camouflage_multimodal_amd/seg_measures.py and of the weighted F-measure's sums.

The measures here never go through a histogram: every count is a sum over a boolean pixel array, every moment an int64 sum over the
pixels, every decision a comparison of Python integers, and the quotients are float64 as the header writes them.  The distance
transform is brute force over all pairs (background pixel, positive pixel) with the header's tie-break.  `table` (the histogram
itself, by np.add.at) exists only to compare the device's table with.
"""
import math
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52


def quantise(pred):
    """q = (int) rintf(fminf(fmaxf(pred, 0), 1) * 255.0f): fp32 multiply, ties to even, NaN -> 0."""
    p = np.asarray(pred, np.float32)
    p = np.where(np.isnan(p), np.float32(0), p)
    p = np.minimum(np.maximum(p, np.float32(0)), np.float32(1))
    prod = p * np.float32(255.0)
    assert prod.dtype == np.float32
    return np.rint(prod).astype(np.int64)


def positive(gt):
    return np.asarray(gt).astype(np.int64) > 127


def rint_ratio(a, b):
    """rint(a / b) of the exact rational, a half to the even neighbour (Python rounds a Fraction that way)."""
    return int(round(Fraction(int(a), int(b))))


def split_point(gt):
    """(X, Y) of one [H, W] mask."""
    g = positive(gt)
    H, W = g.shape
    ys, xs = np.nonzero(g)
    if len(ys) == 0:
        return rint_ratio(W, 2) + 1, rint_ratio(H, 2) + 1
    return rint_ratio(int(xs.sum()), len(xs)) + 1, rint_ratio(int(ys.sum()), len(ys)) + 1


def quadrants(H, W, X, Y):
    return [(slice(0, Y), slice(0, X)), (slice(0, Y), slice(X, W)), (slice(Y, H), slice(0, X)), (slice(Y, H), slice(X, W))]


def table(pred, gt):
    """(hist int32 [N, 4, 2, 256], split int32 [N, 2]) of a batch [N, H, W]: what camo_seg_histograms must give, exactly."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    N, H, W = pred.shape
    hist, split = np.zeros((N, 4, 2, 256), np.int32), np.zeros((N, 2), np.int32)
    for i in range(N):
        q, g = quantise(pred[i]), positive(gt[i])
        X, Y = split_point(gt[i])
        split[i] = X, Y
        for k, sl in enumerate(quadrants(H, W, X, Y)):
            np.add.at(hist[i, k], (g[sl].astype(np.int64).ravel(), q[sl].ravel()), 1)
    return hist, split


def _phi(a, b):
    t = 2.0 * a * b / (a * a + b * b + EPS) + 1.0
    return t * t / 4.0


def f_beta(tp, fp, g):
    pn = tp + fp
    if tp == 0 and pn + g > 0:
        return 0.0
    p = tp / pn if pn else 1.0
    r = tp / g if g else 1.0
    return 1.3 * p * r / (0.3 * p + r)


def e_phi(tp, fp, fn, tn):
    n, g, pn = tp + fp + fn + tn, tp + fn, tp + fp
    if g == 0:
        return (n - pn) / (n - 1 + EPS)
    if g == n:
        return pn / (n - 1 + EPS)
    mp, mg = pn / n, g / n
    return (tp * _phi(1.0 - mp, 1.0 - mg) + fp * _phi(1.0 - mp, -mg) + fn * _phi(-mp, 1.0 - mg) + tn * _phi(-mp, -mg)) / (n - 1 + EPS)


def _confusion(b, g):
    return int((b & g).sum()), int((b & ~g).sum()), int((~b & g).sum()), int((~b & ~g).sum())


def _object(qv, background):
    """o of the header for the q values of one class (the positive class: p; the background class: 1 - p)."""
    c, s, s2 = int(qv.size), int(qv.sum()), int((qv * qv).sum())
    x = (255 * c - s) / (255 * c) if background else s / (255 * c)
    sigma = math.sqrt((c * s2 - s * s) / (65025 * c * (c - 1))) if c > 1 else 0.0
    return 2.0 * x / (x * x + 1.0 + sigma + EPS)


def _ssim(q, g):
    m = int(q.size)
    s, s2, gk, s1 = int(q.sum()), int((q * q).sum()), int(g.sum()), int(q[g].sum())
    x, y = s / (255 * m), gk / m
    nxx, nyy, nxy = m * s2 - s * s, m * gk - gk * gk, m * s1 - s * gk
    den = m - 1 + EPS
    sx, sy, sxy = (nxx / (65025 * m)) / den, (nyy / m) / den, (nxy / (255 * m)) / den
    a = 4.0 * x * y * sxy
    b = (x * x + y * y) * (sx + sy)
    if s != 0 and gk != 0 and nxy != 0:
        return a / (b + EPS)
    if (s == 0 and gk == 0) or (nxx == 0 and nyy == 0):
        return 1.0
    return 0.0


def measures(pred, gt):
    """The header's measures of ONE image [H, W], from the pixels: dict with s_measure, e_max, e_mean, e_adp, f_max, f_mean, f_adp,
    mae_u8, f_curve, e_curve."""
    q, g = quantise(pred), positive(gt)
    H, W = q.shape
    n, G, Q = H * W, int(g.sum()), int(q.sum())
    out = {"mae_u8": int(np.abs(q - 255 * g.astype(np.int64)).sum()) / (255 * n)}
    f_curve, e_curve = [], []
    for t in range(256):
        tp, fp, fn, tn = _confusion(q >= t, g)
        f_curve.append(f_beta(tp, fp, G))
        e_curve.append(e_phi(tp, fp, fn, tn))
    tp, fp, fn, tn = _confusion(q * n >= min(2 * Q, 255 * n), g)
    fs = es = 0.0
    for t in range(256):
        fs += f_curve[t]
        es += e_curve[t]
    out.update(f_curve=f_curve, e_curve=e_curve, f_max=max(f_curve), f_mean=fs / 256.0, f_adp=f_beta(tp, fp, G) if tp else 0.0,
               e_max=max(e_curve), e_mean=es / 256.0, e_adp=e_phi(tp, fp, fn, tn))
    if G == 0:
        out["s_measure"] = 1.0 - Q / (255 * n)
    elif G == n:
        out["s_measure"] = Q / (255 * n)
    else:
        u = G / n
        s_o = u * _object(q[g], False) + (1.0 - u) * _object(q[~g], True)
        X, Y = split_point(gt)
        s_r = 0.0
        for sl in quadrants(H, W, X, Y):
            if q[sl].size:
                s_r += (q[sl].size / n) * _ssim(q[sl], g[sl])
        out["s_measure"] = max(0.0, 0.5 * s_o + 0.5 * s_r)
    return out


def gaussian_7x7():
    k = [math.exp(-(dx * dx + dy * dy) / 50.0) for dy in range(-3, 4) for dx in range(-3, 4)]
    s = 0.0
    for v in k:
        s += v
    return np.array([v / s for v in k], np.float64).reshape(7, 7)


def distance_transform(g, reverse_ties=False):
    """Brute force over all pairs: (d2 int64 [H, W], index int64 [H, W] = y' * W + x' of the nearest positive pixel) of a boolean mask
    with at least one positive pixel; ties to the smaller (y', x') in row-major order (to the LARGER with reverse_ties, which exists
    so that a test can show that the rule matters)."""
    H, W = g.shape
    ys, xs = np.nonzero(g)                                        # row-major order
    assert len(ys) > 0
    d2, idx = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for y in range(H):
        d = (y - ys[None, :]) ** 2 + (np.arange(W)[:, None] - xs[None, :]) ** 2          # [W, positives]
        j = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1) if reverse_ties else np.argmin(d, axis=1)
        d2[y] = d[np.arange(W), j]
        idx[y] = ys[j] * W + xs[j]
    return d2, idx


def weighted_f_sums(pred, gt, reverse_ties=False):
    """(n_fg, A_fg, A_bg) of ONE image [H, W] as Python integers."""
    q, g = quantise(pred), positive(gt)
    H, W = q.shape
    if not g.any():
        return 0, 0, 0
    E = np.abs(q.astype(np.float64) / 255.0 - g.astype(np.float64))
    d2, idx = distance_transform(g, reverse_ties)
    Et = np.where(g, E, E.ravel()[idx])
    pad = np.zeros((H + 6, W + 6), np.float64)
    pad[3:3 + H, 3:3 + W] = Et
    K = gaussian_7x7()
    EA = np.zeros((H, W), np.float64)
    for j in range(7):
        for i in range(7):
            EA += K[j, i] * pad[j:j + H, i:i + W]
    m = np.where(g, np.minimum(E, EA), E)
    B = np.where(g, 1.0, 2.0 - np.exp(math.log(0.5) / 5.0 * np.sqrt(d2.astype(np.float64))))
    fix = np.rint(m * B * 4294967296.0).astype(np.int64)
    return int(g.sum()), int(fix[g].sum()), int(fix[~g].sum())


def weighted_f(nfg, afg, abg):
    if nfg == 0:
        return 0.0
    a_fg, a_bg = afg / 2.0 ** 32, abg / 2.0 ** 32
    tpw = nfg - a_fg
    r = 1.0 - a_fg / nfg
    p = tpw / (tpw + a_bg + EPS)
    return 2.0 * r * p / (r + p + EPS)
