"""include/camo_instances.h restated in plain numpy: the checker of the instance kernels (tests/test_instances.py).

Flood fill with an explicit stack, pixel by pixel in reading order, nothing shared with the kernels' union-find; no scipy in here
(tests/test_instances.py holds this file to scipy.ndimage where that is installed).
"""
import numpy as np

FIELDS, COUNTS = 8, 4
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def quantise(pred):
    """The 8-bit value of include/camo_seg_measures.h: clamp to [0, 1] (a NaN to 0), one fp32 multiply by 255, ties to even."""
    p = np.asarray(pred, np.float32)
    p = np.where(np.isnan(p), np.float32(0), p)
    p = np.minimum(np.maximum(p, np.float32(0)), np.float32(1))
    return np.rint(p * np.float32(255)).astype(np.int64)


def components(mask, connectivity):
    """Connected components of a bool [H, W] mask: (labels int32 with 1 .. C in the reading order of every component's first
    pixel and 0 elsewhere, C)."""
    assert connectivity in (4, 8)
    nb = N8 if connectivity == 8 else N4
    H, W = mask.shape
    labels = np.zeros((H, W), np.int32)
    count = 0
    for y0 in range(H):
        for x0 in range(W):
            if not mask[y0, x0] or labels[y0, x0]:
                continue
            count += 1
            labels[y0, x0] = count
            stack = [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in nb:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and mask[v, u] and not labels[v, u]:
                        labels[v, u] = count
                        stack.append((v, u))
    return labels, count


def fill_holes(mask, connectivity):
    """(the mask with its holes made foreground, the number of holes): a hole is a component of the background, taken with the
    complementary connectivity, with no pixel in the first or last row or column."""
    bg, n = components(~mask, 4 if connectivity == 8 else 8)
    edge = set(bg[0].tolist()) | set(bg[-1].tolist()) | set(bg[:, 0].tolist()) | set(bg[:, -1].tolist())
    holes = [k for k in range(1, n + 1) if k not in edge]
    return mask | np.isin(bg, holes), len(holes)


def instances_image(pred, threshold=0.5, connectivity=8, min_area=0, fill=False, max_instances=64):
    """One [H, W] fp32 map -> (labels int32 [H, W], clean uint8 [H, W], table int64 [max_instances, 8], counts int32 [4])."""
    pred = np.asarray(pred, np.float32)
    H, W = pred.shape
    with np.errstate(invalid="ignore"):
        mask = pred > np.float32(threshold)                 # (a NaN compares false)
    holes = 0
    if fill:
        mask, holes = fill_holes(mask, connectivity)
    raw, n = components(mask, connectivity)
    areas = np.bincount(raw.ravel(), minlength=n + 1)
    keep = np.zeros(n + 1, bool)
    keep[1:] = areas[1:] >= min_area
    new_id = np.zeros(n + 1, np.int32)
    new_id[keep] = np.arange(1, int(keep.sum()) + 1)         # (dropping components keeps the others' reading order)
    labels = new_id[raw]
    K = int(keep.sum())
    q = quantise(pred)
    yy, xx = np.mgrid[:H, :W]
    table = np.zeros((max_instances, FIELDS), np.int64)
    for k in range(1, min(K, max_instances) + 1):
        m = labels == k
        table[k - 1] = (m.sum(), xx[m].min(), yy[m].min(), xx[m].max(), yy[m].max(), xx[m].sum(), yy[m].sum(), q[m].sum())
    counts = np.array([K, n - K, holes, int((labels > 0).sum())], np.int32)
    return labels, (labels > 0).astype(np.uint8), table, counts


def instances(pred, threshold=0.5, connectivity=8, min_area=0, fill=False, max_instances=64):
    """A batch [N, H, W], image by image -> (labels [N, H, W], clean [N, H, W], table [N, max_instances, 8], counts [N, 4])."""
    parts = [instances_image(p, threshold, connectivity, min_area, fill, max_instances) for p in np.asarray(pred, np.float32)]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))
