"""include/camo_split_geo.h restated sequentially in numpy (a helper module, not a conftest): tests/split_ref.py's distance
transform and cores, then ONE heap Dijkstra per split id on the key (path cost, new id), the first-part rule, and the table as
split_ref builds it.  Nothing here is tiled and nothing is iterated to convergence: the kernels' rounds, flags and LDS sweeps are held
to it byte for byte by tests/test_split_geo.py.
"""
import heapq

import numpy as np

from instances_ref import N8, quantise
from split_ref import COUNTS, FIELDS, MAX_ID, cores, distance2, read_ids

STRAIGHT, DIAGONAL = 5, 7


def grow(mine, seeds):
    """``mine`` bool [H, W]: the pixels of one id; ``seeds`` {(y, x): new id} on its kept cores -> {(y, x): (cost, new id)} of every
    pixel a core reaches, by Dijkstra on the tuple: a pixel is settled with the smallest (cost, new id) any path offers it."""
    H, W = mine.shape
    done = {}
    heap = [(0, k, y, x) for (y, x), k in seeds.items()]
    heapq.heapify(heap)
    while heap:
        g, k, y, x = heapq.heappop(heap)
        if (y, x) in done:
            continue
        done[(y, x)] = (g, k)
        for dy, dx in N8:
            v, u = y + dy, x + dx
            if 0 <= v < H and 0 <= u < W and mine[v, u] and (v, u) not in done:
                heapq.heappush(heap, (g + (STRAIGHT if dy == 0 or dx == 0 else DIAGONAL), k, v, u))
    return done


def split_image(labels, pred=None, ratio=(7, 10), min_core=0, max_split=4, max_instances=64):
    """One [H, W] map -> (out int32 [H, W], table int64 [max_instances, 8], counts int32 [4], info): steps 1 - 3, 4g, 5 - 8.  info:
    "core" (the core map), "kept", "core_ids", "split", "new_of" {core number: new id} of the split ids' kept cores, "cost" (per
    pixel of a split id its path cost, -1 where no core reaches and elsewhere)."""
    num, den = ratio
    lab = read_ids(labels)
    H, W = lab.shape
    number, ids, areas, firsts = cores(lab, distance2(lab), num, den)
    kept = [c for c in range(1, len(ids) + 1) if areas[c - 1] >= min_core]
    by_id = {}
    for c in kept:
        by_id.setdefault(ids[c - 1], []).append(c)
    qualifying = sorted(i for i, cs in by_id.items() if len(cs) >= 2)
    split = qualifying[:max_split]
    out = np.zeros((H, W), np.int32)
    cost = np.full((H, W), -1, np.int64)
    new_of, nxt = {}, 0
    for i in range(1, MAX_ID + 1):
        mine = lab == i
        if not mine.any():
            continue
        if i not in split:
            nxt += 1
            out[mine] = nxt
            continue
        mine_new = {c: nxt + k + 1 for k, c in enumerate(by_id[i])}
        new_of.update(mine_new)
        seeds = {(int(y), int(x)): mine_new[int(number[y, x])] for y, x in zip(*np.nonzero(np.isin(number, by_id[i])))}
        out[mine] = nxt + 1                                    # the first part, where no core reaches
        for (y, x), (g, k) in grow(mine, seeds).items():
            out[y, x], cost[y, x] = k, g
        nxt += len(by_id[i])
    K = nxt
    q = quantise(pred) if pred is not None else np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[:H, :W]
    table = np.zeros((max_instances, FIELDS), np.int64)
    for k in range(1, min(K, max_instances) + 1):
        m = out == k
        table[k - 1] = (m.sum(), xx[m].min(), yy[m].min(), xx[m].max(), yy[m].max(), xx[m].sum(), yy[m].sum(), q[m].sum())
    counts = np.array([K, len(split), len(ids) - len(kept), len(qualifying) - len(split)], np.int32)
    assert counts.shape == (COUNTS,)
    info = {"core": number, "kept": kept, "core_ids": ids, "split": split, "qualifying": qualifying, "new_of": new_of, "cost": cost}
    return out, table, counts, info


def split(labels, pred=None, ratio=(7, 10), min_core=0, max_split=4, max_instances=64):
    """A batch [N, H, W], image by image -> {"labels", "table", "counts"} as the call writes them, and "info": the per-image dicts."""
    labels = np.asarray(labels)
    parts = [split_image(l, None if pred is None else pred[n], ratio, min_core, max_split, max_instances) for n, l in enumerate(labels)]
    return {"labels": np.stack([p[0] for p in parts]), "table": np.stack([p[1] for p in parts]), "counts": np.stack([p[2] for p in parts]),
            "info": [p[3] for p in parts]}
