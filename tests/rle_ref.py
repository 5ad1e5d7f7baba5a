"""include/camo_rle.h restated in numpy: the runs of a label map along COCO's column-major order, the counts of one
id, the label map of a list of annotations, and COCO's string form of the counts one count at a time.  Integers only; the kernels and
camouflage_multimodal_amd/rle.py are held to this file byte for byte."""
import numpy as np


def runs_image(labels, R):
    """(runs int32 [R, 2], counts int32 [2]) of one [H, W] map: (start, label) of every maximal run along p = x H + y."""
    flat = np.asarray(labels).astype(np.int32).flatten(order="F")
    heads = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1]).astype(np.int64)
    M, wrote = heads.size, min(heads.size, R)
    runs = np.zeros((R, 2), np.int32)
    runs[:wrote, 0], runs[:wrote, 1] = heads[:wrote], flat[heads[:wrote]]
    return runs, np.array([M, wrote], np.int32)


def runs_batch(labels, R):
    both = [runs_image(l, R) for l in labels]
    return {"runs": np.stack([b[0] for b in both]), "counts": np.stack([b[1] for b in both])}


def runs_by_loop(labels):
    """[(start, label)] with a plain loop over the positions."""
    H, W = labels.shape
    out = []
    for p in range(H * W):
        y, x = p % H, p // H
        if p == 0 or labels[y, x] != labels[(p - 1) % H, (p - 1) // H]:
            out.append((p, int(labels[y, x])))
    return out


def mask_counts(mask):
    """COCO's counts of one binary [H, W] mask: run lengths along p, the first one background (0 when the mask owns position 0)."""
    flat = np.asarray(mask).astype(bool).flatten(order="F")
    heads = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]])
    counts = np.diff(heads)
    return np.concatenate([[0], counts]) if flat[0] else counts


def label_counts(labels):
    """{id: counts} of every id > 0 of one [H, W] map."""
    return {int(i): mask_counts(labels == i) for i in np.unique(labels) if i > 0}


def counts_mask(counts, H, W):
    """The inverse of mask_counts (the counts must sum to H W)."""
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    assert flat.size == H * W
    return flat.reshape(H, W, order="F")


def decode(cnts, ann_off, ann_image, ann_value, N, H, W):
    """(labels int32 [N, H, W], ann_sum int64 [A]) of include/camo_rle.h's camo_rle_decode, one position at a time per run."""
    labels = np.zeros((N, H * W), np.int32)
    A = len(ann_image)
    ann_sum = np.zeros(A, np.int64)
    for a in range(A):
        c = np.asarray(cnts[ann_off[a]:ann_off[a + 1]], np.int64)
        if (c < 0).any() or not 0 <= ann_image[a] < N or ann_value[a] < 1:
            ann_sum[a] = -1
            continue
        ann_sum[a] = c.sum()
        at = 0
        for k, n in enumerate(c):
            if k % 2 == 1:
                lo, hi = min(at, H * W), min(at + int(n), H * W)
                row = labels[ann_image[a]]
                row[lo:hi] = np.maximum(row[lo:hi], ann_value[a])
            at += int(n)
    return labels.reshape(N, W, H).transpose(0, 2, 1).copy(), ann_sum      # (position p = x H + y: [W, H] in memory)


def to_string(cnts):
    """COCO's rleToString, one count and one group at a time."""
    out = []
    for i, c in enumerate(cnts):
        x = int(c) - (int(cnts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            g = x & 31
            x >>= 5
            more = (x != -1) if g & 16 else (x != 0)
            out.append(chr((g | (32 if more else 0)) + 48))
    return "".join(out)


def from_string(s):
    """COCO's rleFrString, one character at a time."""
    cnts, at = [], 0
    while at < len(s):
        x, k, more = 0, 0, True
        while more:
            g = ord(s[at]) - 48
            x |= (g & 31) << (5 * k)
            more = bool(g & 32)
            at += 1
            k += 1
            if not more and g & 16:
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts
