"""include/camo_inst_match.h restated in numpy and plain Python, with no library call: np.add.at builds the overlap table, loops with
fractions.Fraction do the rank and the greedy match.  AP is COCO's 101-point interpolation, restated with numpy."""
from fractions import Fraction

import numpy as np

MAX_IMAGE_PIXELS = 1 << 26      # CAMO_RGD_MAX_IMAGE_PIXELS
COCO = tuple(Fraction(n, 20) for n in range(10, 20))


def blocks(H, W, ids, seed, cell=4):
    """A [H, W] case map of cell x cell blocks with ids 0 .. ids (test_inst_match, test_boundary; test_rle with cell = 3)."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, ids + 1, ((H + cell - 1) // cell, (W + cell - 1) // cell))
    return np.kron(coarse, np.ones((cell, cell), np.int64))[:H, :W]


def score_table(N, rows, seed):
    """A [N, rows, 8] case table as camo_instances writes it: random areas and score sums, the other fields 0."""
    rng = np.random.default_rng(seed)
    area = rng.integers(1, 200, (N, rows))
    t = np.zeros((N, rows, 8), np.int64)
    t[..., 0], t[..., 7] = area, rng.integers(0, 255 * area + 1)
    return t


def overlap(pred, gt, P, G):
    """(inter int64 [P + 1, G + 1], pixels with pred out of 0 .. P, pixels with gt out of 0 .. G) of two [H, W] label maps."""
    pred, gt = np.asarray(pred, np.int64).ravel(), np.asarray(gt, np.int64).ravel()
    pin, gin = (pred >= 0) & (pred <= P), (gt >= 0) & (gt <= G)
    inter = np.zeros((P + 1, G + 1), np.int64)
    both = pin & gin
    np.add.at(inter, (pred[both], gt[both]), 1)
    return inter, int((~pin).sum()), int((~gin).sum())


def scores(table, P):
    """The score of ids 1 .. P as Fractions: Sq / area of a table row that is one, else 0."""
    out = []
    for p in range(1, P + 1):
        s = Fraction(0)
        if table is not None and p <= len(table):
            area, sq = int(table[p - 1][0]), int(table[p - 1][7])
            if 0 < area <= MAX_IMAGE_PIXELS and 0 <= sq <= 255 * area:
                s = Fraction(sq, area)
        out.append(s)
    return out


def match_image(pred, gt, P, G, table=None, thresholds=COCO):
    """One image -> dict of int32 arrays: inter [P + 1, G + 1], pred_rows [P, 4], gt_area [G], match [T, P], gt_match [T, G],
    counts [4]."""
    inter, oob_p, oob_g = overlap(pred, gt, P, G)
    area_p, area_g = inter.sum(axis=1), inter.sum(axis=0)
    sc = scores(table, P)
    order = sorted(range(1, P + 1), key=lambda p: (-sc[p - 1], p))
    rank = {p: r for r, p in enumerate(order)}

    def iou(p, g):
        i = int(inter[p, g])
        return Fraction(i, int(area_p[p]) + int(area_g[g]) - i)

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
    rows = np.zeros((P, 4), np.int32)
    for p in range(1, P + 1):
        best, best_iou = 0, None
        for g in range(1, G + 1):
            if inter[p, g] and (best == 0 or iou(p, g) > best_iou):
                best, best_iou = g, iou(p, g)
        rows[p - 1] = (area_p[p], rank[p], best, inter[p, best] if best else 0)
    counts = np.array([oob_p, oob_g, int((area_p[1:] > 0).sum()), int((area_g[1:] > 0).sum())], np.int32)
    return {"inter": inter.astype(np.int32), "pred_rows": rows, "gt_area": area_g[1:].astype(np.int32), "match": match, "gt_match": gt_match,
            "counts": counts}


def match_batch(pred, gt, P, G, table=None, thresholds=COCO):
    """[N, H, W] maps (and a [N, rows, 8] table), image by image."""
    parts = [match_image(pred[n], gt[n], P, G, None if table is None else table[n], thresholds) for n in range(len(pred))]
    return {k: np.stack([p[k] for p in parts]) for k in parts[0]}


def average_precision(scored, n_gt):
    """101-point AP of [(score, hit)] against n_gt instances; None without ground truth."""
    if n_gt == 0:
        return None
    if not scored:
        return 0.0
    s = np.array([v for v, _ in scored], np.float64)
    hit = np.array([h for _, h in scored], bool)[np.argsort(-s, kind="stable")]
    tp = np.cumsum(hit)
    prec = np.maximum.accumulate((tp / np.arange(1, len(hit) + 1))[::-1])[::-1]
    total = Fraction(0)
    for j in range(101):
        at = np.nonzero(tp * 100 >= j * n_gt)[0]
        if len(at):
            total += Fraction(float(prec[at[0]]))
    return float(total / 101)
