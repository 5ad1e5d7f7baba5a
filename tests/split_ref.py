"""include/camo_split.h restated sequentially in numpy (a helper module, not a conftest): a brute-force distance transform over every
background pixel, a flood fill for the cores, a brute-force nearest site.  Nothing here is separable, tiled or pruned: the kernels'
column and row passes, union-find and outward search are held to it byte for byte by tests/test_split.py.
"""
import numpy as np

from instances_ref import N8, quantise

FIELDS, COUNTS, MAX_ID = 8, 4, 1024


def read_ids(labels):
    """The label map as the call reads it: a value outside 0 .. MAX_ID is background."""
    lab = np.asarray(labels, np.int64)
    return np.where((lab >= 0) & (lab <= MAX_ID), lab, 0)


def distance2(lab):
    """D2 of one [H, W] map of ids: per foreground pixel the smallest squared Euclidean distance to a pixel with id 0 inside the
    image, by looking at every such pixel; 0 on the background; -1 on every foreground pixel when the image has no background."""
    H, W = lab.shape
    by, bx = np.nonzero(lab == 0)
    if len(by) == 0:
        return np.full((H, W), -1, np.int64)
    out = np.zeros((H, W), np.int64)
    fy, fx = np.nonzero(lab > 0)
    for at in range(0, len(fy), 256):
        y, x = fy[at:at + 256, None], fx[at:at + 256, None]
        out[fy[at:at + 256], fx[at:at + 256]] = ((y - by[None]) ** 2 + (x - bx[None]) ** 2).min(axis=1)
    return out


def cores(lab, d2, num, den):
    """(core map int32 [H, W]: 0, or the core's number 1 .. C in the row-major order of the cores' first pixels; the id of every
    core; its area; its first pixel's row-major index), by flood fill with 8 neighbours over core pixels of equal id."""
    H, W = lab.shape
    m2 = np.zeros(MAX_ID + 1, np.int64)
    np.maximum.at(m2, lab.ravel(), d2.ravel())
    core = (lab > 0) & (d2 > 0) & (den * den * d2 > num * num * m2[lab])      # (python / int64 arithmetic: no overflow below 2^62)
    number = np.zeros((H, W), np.int32)
    ids, areas, firsts = [], [], []
    for y0 in range(H):
        for x0 in range(W):
            if not core[y0, x0] or number[y0, x0]:
                continue
            ids.append(int(lab[y0, x0])); areas.append(0); firsts.append(y0 * W + x0)
            c = len(ids)
            number[y0, x0] = c
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                areas[-1] += 1
                for dy, dx in N8:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and core[v, u] and not number[v, u] and lab[v, u] == lab[y0, x0]:
                        number[v, u] = c
                        stack.append((v, u))
    return number, ids, areas, firsts


def split_image(labels, pred=None, ratio=(7, 10), min_core=0, max_split=4, max_instances=64):
    """One [H, W] map -> (out int32 [H, W], table int64 [max_instances, 8], counts int32 [4], info): the header's steps 1 - 8 in
    order.  info: what the tests' property checks read -- "d2", "core" (the core map), "kept" (core numbers), "split" (ids),
    "qualifying" (ids), "site" (per pixel of a split id the row-major index of the site it took, -1 elsewhere)."""
    num, den = ratio
    lab = read_ids(labels)
    H, W = lab.shape
    d2 = distance2(lab)
    number, ids, areas, firsts = cores(lab, d2, num, den)
    kept = [c for c in range(1, len(ids) + 1) if areas[c - 1] >= min_core]
    dropped = len(ids) - len(kept)
    by_id = {}
    for c in kept:                                           # (ascending core number = row-major order of the first pixels)
        by_id.setdefault(ids[c - 1], []).append(c)
    qualifying = sorted(i for i, cs in by_id.items() if len(cs) >= 2)
    split = qualifying[:max_split]
    out = np.zeros((H, W), np.int32)
    site = np.full((H, W), -1, np.int64)
    nxt = 0
    for i in range(1, MAX_ID + 1):
        mine = lab == i
        if not mine.any():
            continue
        if i not in split:
            nxt += 1
            out[mine] = nxt
            continue
        sy, sx = np.nonzero(np.isin(number, by_id[i]))       # the sites in row-major order: the first of the nearest is the rule's
        new_of = {c: nxt + k + 1 for k, c in enumerate(by_id[i])}
        for y, x in zip(*np.nonzero(mine)):
            d = (y - sy) ** 2 + (x - sx) ** 2
            j = int(np.argmin(d))                            # (argmin returns the first minimum: the smallest (y', x'))
            out[y, x] = new_of[int(number[sy[j], sx[j]])]
            site[y, x] = sy[j] * W + sx[j]
        nxt += len(by_id[i])
    K = nxt
    q = quantise(pred) if pred is not None else np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[:H, :W]
    table = np.zeros((max_instances, FIELDS), np.int64)
    for k in range(1, min(K, max_instances) + 1):
        m = out == k
        table[k - 1] = (m.sum(), xx[m].min(), yy[m].min(), xx[m].max(), yy[m].max(), xx[m].sum(), yy[m].sum(), q[m].sum())
    counts = np.array([K, len(split), dropped, len(qualifying) - len(split)], np.int32)
    info = {"d2": d2, "core": number, "kept": kept, "core_ids": ids, "core_areas": areas, "split": split, "qualifying": qualifying, "site": site}
    return out, table, counts, info


def split(labels, pred=None, ratio=(7, 10), min_core=0, max_split=4, max_instances=64):
    """A batch [N, H, W], image by image -> {"labels", "table", "counts"} as the call writes them, and "info": the per-image dicts."""
    labels = np.asarray(labels)
    parts = [split_image(l, None if pred is None else pred[n], ratio, min_core, max_split, max_instances) for n, l in enumerate(labels)]
    return {"labels": np.stack([p[0] for p in parts]), "table": np.stack([p[1] for p in parts]), "counts": np.stack([p[2] for p in parts]),
            "info": [p[3] for p in parts]}
