"""include/camo_boundary.h restated in numpy and plain Python, with no library call (a helper module, not a conftest).

``boundary_labels_ref`` is the window definition itself, a numpy slice per pixel -- not the run form the kernels use.
``boundary_match_ref`` follows inst_match_ref.py: np.add.at builds the two overlap tables, fractions.Fraction takes the smaller of
the two IoUs, tests the thresholds and runs the greedy match."""
from fractions import Fraction

import numpy as np

import inst_match_ref as R

COCO = R.COCO


def boundary_labels_ref(labels, d):
    """[H, W] or [N, H, W] labels -> int32 of the same shape: 0 where the label is <= 0 or the whole (2d + 1)^2 window lies inside the
    image and carries the pixel's label, else the label."""
    labels = np.asarray(labels)
    if labels.ndim == 3:
        return np.stack([boundary_labels_ref(m, d) for m in labels])
    H, W = labels.shape
    out = np.zeros((H, W), np.int32)
    for y in range(H):
        for x in range(W):
            L = int(labels[y, x])
            if L <= 0:
                continue
            inside = y - d >= 0 and y + d < H and x - d >= 0 and x + d < W
            if not (inside and (labels[y - d:y + d + 1, x - d:x + d + 1] == L).all()):
                out[y, x] = L
    return out


def combined(i, u, ib, ub):
    """The smaller of i / u and ib / ub as (numerator, denominator): 0 / 1 when ub is 0, the mask's pair when they are equal."""
    if ub == 0:
        return 0, 1
    return (i, u) if Fraction(i, u) <= Fraction(ib, ub) else (ib, ub)


def boundary_match_image(pred, gt, pred_bd, gt_bd, P, G, table=None, thresholds=COCO):
    """One image -> dict of int32 arrays: inter, inter_bd [P + 1, G + 1], pred_rows [P, 6], gt_area [G, 2], match [T, P],
    gt_match [T, G], counts [4]."""
    inter, oob_p, oob_g = R.overlap(pred, gt, P, G)
    inter_bd, _, _ = R.overlap(pred_bd, gt_bd, P, G)
    area_p, area_g = inter.sum(axis=1), inter.sum(axis=0)
    bd_p, bd_g = inter_bd.sum(axis=1), inter_bd.sum(axis=0)
    sc = R.scores(table, P)
    order = sorted(range(1, P + 1), key=lambda p: (-sc[p - 1], p))
    rank = {p: r for r, p in enumerate(order)}

    def iou(p, g):
        i, ib = int(inter[p, g]), int(inter_bd[p, g])
        n, m = combined(i, int(area_p[p]) + int(area_g[g]) - i, ib, int(bd_p[p]) + int(bd_g[g]) - ib)
        return Fraction(n, m)

    T = len(thresholds)
    match, gt_match = np.zeros((T, P), np.int32), np.zeros((T, G), np.int32)
    for k, t in enumerate(thresholds):
        t = Fraction(t)
        for p in order:
            if area_p[p] == 0:
                continue
            best, best_iou = 0, None
            for g in range(1, G + 1):
                if area_g[g] == 0 or gt_match[k, g - 1] or inter[p, g] == 0:
                    continue
                v = iou(p, g)
                if v >= t and (best == 0 or v > best_iou):
                    best, best_iou = g, v
            if best:
                match[k, p - 1], gt_match[k, best - 1] = best, p
    rows = np.zeros((P, 6), np.int32)
    for p in range(1, P + 1):
        best, best_iou = 0, None
        for g in range(1, G + 1):
            if inter[p, g] and (best == 0 or iou(p, g) > best_iou):
                best, best_iou = g, iou(p, g)
        rows[p - 1] = (area_p[p], rank[p], best, inter[p, best] if best else 0, bd_p[p], inter_bd[p, best] if best else 0)
    counts = np.array([oob_p, oob_g, int((area_p[1:] > 0).sum()), int((area_g[1:] > 0).sum())], np.int32)
    return {"inter": inter.astype(np.int32), "inter_bd": inter_bd.astype(np.int32), "pred_rows": rows,
            "gt_area": np.stack([area_g[1:], bd_g[1:]], axis=1).astype(np.int32), "match": match, "gt_match": gt_match, "counts": counts}


def boundary_match_ref(pred, gt, pred_bd, gt_bd, P, G, table=None, thresholds=COCO):
    """[N, H, W] maps (and a [N, rows, 8] table), image by image."""
    parts = [boundary_match_image(pred[n], gt[n], pred_bd[n], gt_bd[n], P, G, None if table is None else table[n], thresholds)
             for n in range(len(pred))]
    return {k: np.stack([p[k] for p in parts]) for k in parts[0]}
