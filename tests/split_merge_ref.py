"""include/camo_split_merge.h restated sequentially in numpy (a helper module, not a conftest): tests/split_ref.py's brute-force
distance transform, a double loop over the four forward neighbours of every pixel, plain dictionaries for the peaks, the passes and
the links, and a walk up every chain.  Nothing here is tiled, reduced in a wave or jumped: the kernels' LDS tables, packed keys and
pointer jumping are held to it byte for byte by tests/test_split_merge.py.
"""
import numpy as np

from instances_ref import quantise
from split_ref import FIELDS, MAX_ID, distance2, read_ids

COUNTS = 4
FORWARD = ((0, 1), (1, -1), (1, 0), (1, 1))      # E, SW, S, SE: with them every unordered pair of 8-neighbours is met once


def higher(b, a, peak):
    """Is part b higher than part a?"""
    return peak[b] > peak[a] or (peak[b] == peak[a] and b < a)


def merge_image(labels, parts, pred=None, merge=(4, 5), max_instances=64):
    """One [H, W] pair -> (out int32 [H, W], table int64 [max_instances, 8], counts int32 [4], info): the header's steps 1 - 10 in
    order.  info: what the tests' property checks read -- "d2", "peak" {part: peak}, "contacts" {(lower, higher): the largest value
    between the two}, "pass" {part: (value, up)}, "links" {part: up} of the linked parts, "new_of" {part: new id}."""
    num, den = merge
    lab = read_ids(labels)
    prt = np.asarray(parts, np.int64)
    H, W = lab.shape
    fg = lab > 0
    table = np.zeros((max_instances, FIELDS), np.int64)
    if (fg & ((prt < 1) | (prt > MAX_ID))).any():                                      # step 10
        return np.where(fg, prt, 0).astype(np.int32), table, np.array([-1, 0, 0, 0], np.int32), {"supported": False}
    d2 = distance2(lab)
    peak, owner = {}, {}
    for y in range(H):
        for x in range(W):
            if fg[y, x]:
                a = int(prt[y, x])
                peak[a] = max(peak.get(a, -1), int(d2[y, x]))
                owner[a] = max(owner.get(a, 0), int(lab[y, x]))
    contacts = {}
    if (lab == 0).any():                                                               # (no background: no D2, no contact, no link)
        for y in range(H):
            for x in range(W):
                if not fg[y, x]:
                    continue
                for dy, dx in FORWARD:
                    v, u = y + dy, x + dx
                    if not (0 <= v < H and 0 <= u < W) or lab[v, u] != lab[y, x] or prt[v, u] == prt[y, x]:
                        continue
                    a, b = int(prt[y, x]), int(prt[v, u])
                    pair = (a, b) if higher(b, a, peak) else (b, a)
                    contacts[pair] = max(contacts.get(pair, 0), int(min(d2[y, x], d2[v, u])))
    best = {}
    for (a, b), value in contacts.items():                                             # step 4: the largest value, a tie to the smaller part
        if a not in best or (value, -b) > (best[a][0], -best[a][1]):
            best[a] = (value, b)
    links = {a: b for a, (value, b) in best.items() if den * den * value >= num * num * peak[a]}
    root = {}
    for a in peak:
        r = a
        while r in links:
            assert higher(links[r], r, peak)
            r = links[r]
        root[a] = r
    groups = {}
    for a in sorted(peak):
        groups.setdefault(root[a], []).append(a)
    order = sorted(groups.values(), key=lambda g: g[0])
    new_of = {a: k + 1 for k, g in enumerate(order) for a in g}
    out = np.zeros((H, W), np.int32)
    for y, x in zip(*np.nonzero(fg)):
        out[y, x] = new_of[int(prt[y, x])]
    K = len(order)
    q = quantise(pred) if pred is not None else np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[:H, :W]
    for k in range(1, min(K, max_instances) + 1):
        m = out == k
        table[k - 1] = (m.sum(), xx[m].min(), yy[m].min(), xx[m].max(), yy[m].max(), xx[m].sum(), yy[m].sum(), q[m].sum())
    owned = {}
    for a, o in owner.items():
        owned.setdefault(o, []).append(a)
    whole = sum(1 for ps in owned.values() if len(ps) >= 2 and len({root[a] for a in ps}) == 1)
    counts = np.array([K, len(peak), sum(1 for g in order if len(g) >= 2), whole], np.int32)
    assert counts.shape == (COUNTS,)
    info = {"supported": True, "d2": d2, "peak": peak, "contacts": contacts, "pass": best, "links": links, "new_of": new_of}
    return out, table, counts, info


def merge(labels, parts, pred=None, merge=(4, 5), max_instances=64):
    """A batch [N, H, W], image by image -> {"labels", "table", "counts"} as the call writes them, and "info": the per-image dicts."""
    labels, parts = np.asarray(labels), np.asarray(parts)
    res = [merge_image(l, parts[n], None if pred is None else pred[n], merge, max_instances) for n, l in enumerate(labels)]
    return {"labels": np.stack([r[0] for r in res]), "table": np.stack([r[1] for r in res]), "counts": np.stack([r[2] for r in res]),
            "info": [r[3] for r in res]}
