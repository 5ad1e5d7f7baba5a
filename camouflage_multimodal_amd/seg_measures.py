"""The camouflaged-object benchmark measures on MI355X (include/camo_seg_measures.h): S-alpha, E-phi, the F-beta
curve and the weighted F-measure of a predicted map against a ground-truth mask.

The device sums integers -- ``segmentation_histograms`` gives the 256-bin table of the 8-bit prediction split by ground truth and by
the S-measure's quadrants, ``weighted_f_sums`` the three sums behind F-beta-w -- and this module takes the ratios from them on the
host: Python integers for every sum and every decision, float64 for the quotients, exactly as the header writes them.
PARITY UNPINNED: the reference's utils/metrics.py and the usual toolkits cannot be read here, so the header's text is the
definition.  A map is not min-max normalised; do that in torch first if it is wanted.  There is no CPU path: tensors that are not
on a HIP device raise.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, image_planes, workspace

EPS = 2.0 ** -52
MEASURE_KEYS = ("s_measure", "e_max", "e_mean", "e_adp", "f_max", "f_mean", "f_adp", "mae_u8")


def _planes(pred, gt):
    """pred fp32 [N, H, W] readable in place (a channel of [N, C, H, W] is), its image stride, and gt as contiguous uint8."""
    _lib.require_device(pred, "pred")
    _lib.require_device(gt, "gt")
    if pred.dim() == 2:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
    if pred.dim() != 3 or gt.shape != pred.shape or pred.numel() == 0:
        raise ValueError(f"need pred [N, H, W] and gt of the same shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    N, H, W = pred.shape
    if H * W < 2:
        raise ValueError("the measures need at least two pixels per image")
    pred, stride = image_planes(pred)
    g = gt.to(device=pred.device)
    g = (g.to(torch.uint8) * 255 if g.dtype == torch.bool else g.to(torch.uint8)).contiguous()
    return pred, stride, g


@torch.no_grad()
def segmentation_histograms(pred, gt):
    """The table of ``camo_seg_histograms``: ``pred`` fp32 [N, H, W] (or [H, W]; one channel of a [N, C, H, W] map is read in place),
    ``gt`` [N, H, W] uint8 (positive above 127) or bool -> (hist int32 [N, 4, 2, 256], split int32 [N, 2] = (X, Y)) on the device:
    hist[i, k, g, q] pixels of image i in quadrant k with ground truth g and 8-bit value q.  Integer sums: two calls give the same bytes."""
    pred, stride, g = _planes(pred, gt)
    N, H, W = pred.shape
    dev = pred.device
    hist = torch.empty(N, _lib.SEG_QUADRANTS, 2, _lib.SEG_BINS, dtype=torch.int32, device=dev)
    split = torch.empty(N, 2, dtype=torch.int32, device=dev)
    call("camo_seg_histograms", dev, _ptr(pred), stride, _ptr(g), N, H, W, _ptr(hist), _ptr(split), _stream_ptr(dev))
    return hist, split


def gaussian_7x7():
    """The 49 doubles ``camo_seg_weighted_f`` takes: exp(-(dx^2 + dy^2) / (2 * 5^2)), dx, dy = -3..3, row-major, divided by their sum
    (added in that order)."""
    k = [math.exp(-(dx * dx + dy * dy) / 50.0) for dy in range(-3, 4) for dx in range(-3, 4)]
    s = 0.0
    for v in k:
        s += v
    return [v / s for v in k]


@torch.no_grad()
def weighted_f_sums(pred, gt):
    """``camo_seg_weighted_f``: int64 [N, 3] = (n_fg, A_fg, A_bg) on the device (``pred`` and ``gt`` as for ``segmentation_histograms``)."""
    pred, stride, g = _planes(pred, gt)
    N, H, W = pred.shape
    if max(H, W) > _lib.SEG_WF_MAX_SIDE:
        raise ValueError(f"the weighted F-measure takes images of at most {_lib.SEG_WF_MAX_SIDE} pixels a side, got {H} x {W}")
    dev = pred.device
    ws, nbytes = workspace("camo_seg_weighted_f_workspace_bytes", N, H, W, device=dev,
                           refuse=lambda: _lib.CamoError(f"camo_seg_weighted_f does not support N = {N}, H = {H}, W = {W}"))
    gauss = torch.tensor(gaussian_7x7(), dtype=torch.float64, device=dev)
    sums = torch.empty(N, 3, dtype=torch.int64, device=dev)
    call("camo_seg_weighted_f", dev, _ptr(pred), stride, _ptr(g), N, H, W, _ptr(gauss), _ptr(ws), nbytes, _ptr(sums), _stream_ptr(dev))
    return sums


def weighted_f_from_sums(sums):
    """The header's ratio of every (n_fg, A_fg, A_bg) row (tensor or nested list), in float64; 0 when there is no positive pixel."""
    rows = sums.tolist() if isinstance(sums, torch.Tensor) else [list(r) for r in sums]
    out = []
    for nfg, afg, abg in rows:
        nfg = int(nfg)
        if nfg == 0:
            out.append(0.0)
            continue
        a_fg, a_bg = int(afg) / 2.0 ** _lib.RGD_FIX_BITS, int(abg) / 2.0 ** _lib.RGD_FIX_BITS
        tpw = nfg - a_fg
        r = 1.0 - a_fg / nfg
        p = tpw / (tpw + a_bg + EPS)
        out.append(2.0 * r * p / (r + p + EPS))
    return out


def weighted_f_measure(pred, gt):
    """F-beta-w of every image: a list of floats (one host copy, of the [N, 3] sums)."""
    return weighted_f_from_sums(weighted_f_sums(pred, gt))


def _phi(a, b):
    t = 2.0 * a * b / (a * a + b * b + EPS) + 1.0
    return t * t / 4.0


def _f_beta(tp, pn, g):
    if tp == 0 and pn + g > 0:
        return 0.0
    p = tp / pn if pn else 1.0
    r = tp / g if g else 1.0
    return 1.3 * p * r / (0.3 * p + r)


def _e_phi(tp, fp, fn, tn, n):
    g, pn = tp + fn, tp + fp
    if g == 0:
        return (n - pn) / (n - 1 + EPS)
    if g == n:
        return pn / (n - 1 + EPS)
    mp, mg = pn / n, g / n
    return (tp * _phi(1.0 - mp, 1.0 - mg) + fp * _phi(1.0 - mp, -mg) + fn * _phi(-mp, 1.0 - mg) + tn * _phi(-mp, -mg)) / (n - 1 + EPS)


def _object(x, c, s, s2):
    sigma = math.sqrt((c * s2 - s * s) / (65025 * c * (c - 1))) if c > 1 else 0.0
    return 2.0 * x / (x * x + 1.0 + sigma + EPS)


def _ssim(m, s, s2, gk, s1):
    x, y = s / (255 * m), gk / m
    nxx, nyy, nxy = m * s2 - s * s, m * gk - gk * gk, m * s1 - s * gk
    den = m - 1 + EPS
    sx, sy, sxy = (nxx / (65025 * m)) / den, (nyy / m) / den, (nxy / (255 * m)) / den
    a = 4.0 * x * y * sxy
    b = (x * x + y * y) * (sx + sy)
    if s != 0 and gk != 0 and nxy != 0:
        return a / (b + EPS)
    return 1.0 if (s == 0 and gk == 0) or (nxx == 0 and nyy == 0) else 0.0


def _image_measures(table, n, curves):
    """``table`` [4][2][256] Python integers of one image of n pixels."""
    h = [[sum(table[k][g][q] for k in range(4)) for q in range(256)] for g in range(2)]
    if sum(h[0]) + sum(h[1]) != n:
        raise ValueError(f"the table holds {sum(h[0]) + sum(h[1])} pixels, H * W is {n}")
    G = sum(h[1])
    q0 = sum(q * c for q, c in enumerate(h[0]))
    q1 = sum(q * c for q, c in enumerate(h[1]))
    Q = q0 + q1
    out = {"mae_u8": (q0 + 255 * G - q1) / (255 * n)}
    # the curves: TP and FP at t from the top bin down
    f_curve, e_curve = [0.0] * 256, [0.0] * 256
    tp = fp = 0
    for t in range(255, -1, -1):
        tp += h[1][t]
        fp += h[0][t]
        f_curve[t] = _f_beta(tp, tp + fp, G)
        e_curve[t] = _e_phi(tp, fp, G - tp, n - G - fp, n)
    bound = min(2 * Q, 255 * n)
    ta = -(-bound // n)                                           # the least t with t n >= bound
    tpa, fpa = sum(h[1][ta:]), sum(h[0][ta:])
    fs = es = 0.0
    for t in range(256):
        fs += f_curve[t]
        es += e_curve[t]
    out.update(f_max=max(f_curve), f_mean=fs / 256.0, f_adp=_f_beta(tpa, tpa + fpa, G) if tpa else 0.0,
               e_max=max(e_curve), e_mean=es / 256.0, e_adp=e_curve[ta])
    if G == 0:
        out["s_measure"] = 1.0 - Q / (255 * n)
    elif G == n:
        out["s_measure"] = Q / (255 * n)
    else:
        u, B = G / n, n - G
        s_o = u * _object(q1 / (255 * G), G, q1, sum(q * q * c for q, c in enumerate(h[1]))) \
            + (1.0 - u) * _object((255 * B - q0) / (255 * B), B, q0, sum(q * q * c for q, c in enumerate(h[0])))
        s_r = 0.0
        for k in range(4):
            m = sum(table[k][0]) + sum(table[k][1])
            if m == 0:
                continue
            s = sum(q * (table[k][0][q] + table[k][1][q]) for q in range(256))
            s2 = sum(q * q * (table[k][0][q] + table[k][1][q]) for q in range(256))
            s_r += (m / n) * _ssim(m, s, s2, sum(table[k][1]), sum(q * c for q, c in enumerate(table[k][1])))
        out["s_measure"] = max(0.0, 0.5 * s_o + 0.5 * s_r)
    if curves:
        out["f_curve"], out["e_curve"] = f_curve, e_curve
    return out


def cod_measures(hist, split, H, W, curves=False):
    """The measures of include/camo_seg_measures.h from ``segmentation_histograms``' table (tensors or nested lists), on the host: a
    list of dicts, one per image, with s_measure, e_max, e_mean, e_adp, f_max, f_mean, f_adp, mae_u8 and the split point, plus the
    256-entry f_curve and e_curve with ``curves=True``.  Every sum and every decision is taken in Python integers."""
    tables = hist.tolist() if isinstance(hist, torch.Tensor) else hist        # (a device tensor: the one copy)
    splits = split.tolist() if isinstance(split, torch.Tensor) else split
    out = []
    for table, xy in zip(tables, splits):
        table = [[[int(v) for v in row] for row in quad] for quad in table]
        m = _image_measures(table, int(H) * int(W), curves)
        m["split"] = (int(xy[0]), int(xy[1]))
        out.append(m)
    return out


def aggregate_cod_measures(measures):
    """A dataset's numbers from its images' dicts (``cod_measures(..., curves=True)``): the F and E curves are averaged over the images
    and the maximum and the mean taken of the averaged curves; s_measure, e_adp, f_adp, mae_u8 (and wf where every image has it) are
    averaged over the images."""
    measures = list(measures)
    if not measures:
        raise ValueError("aggregate_cod_measures needs at least one image")
    if any("f_curve" not in m or "e_curve" not in m for m in measures):
        raise ValueError("aggregate_cod_measures needs the curves: call cod_measures(..., curves=True)")
    k = float(len(measures))
    out = {}
    for name in ("f", "e"):
        curve = [sum(m[name + "_curve"][t] for m in measures) / k for t in range(256)]
        out[name + "_curve"] = curve
        out[name + "_max"] = max(curve)
        out[name + "_mean"] = sum(curve) / 256.0
    for key in ("s_measure", "e_adp", "f_adp", "mae_u8") + (("wf",) if all("wf" in m for m in measures) else ()):
        out[key] = sum(m[key] for m in measures) / k
    return out


def cod_metrics(pred, gt, curves=False):
    """Everything above for a batch: ``cod_measures`` of ``segmentation_histograms`` with ``wf`` = ``weighted_f_measure`` added."""
    hist, split = segmentation_histograms(pred, gt)
    sums = weighted_f_sums(pred, gt)
    H, W = pred.shape[-2:]
    out = cod_measures(hist, split, H, W, curves)
    for m, wf in zip(out, weighted_f_from_sums(sums)):
        m["wf"] = wf
    return out
