"""include/camo_poly.h restated in numpy, SEQUENTIALLY as COCO's rleFrPoly runs: the point lists u, v of all edges
back to back, the loop over consecutive pairs with the float64 (xd + .5) / 5 - .5 arithmetic and floor / ceil, then the sort, the
differences and the zero-count merge into counts.  Deliberately not the per-edge integer form the kernels use.  The annotation rules
5 - 7 (union, largest value wins, areas, invalid annotations) follow.  The kernels are held to this file byte for byte."""
from fractions import Fraction

import numpy as np

MARGIN = 1024
SCALE = 5.0


def scaled_vertices(poly):
    """(X, Y) int64 of a flat [x0, y0, x1, y1, ...] or [k, 2] polygon: (int)(5.0 * c + 0.5), the first vertex appended again."""
    c = np.asarray(poly, np.float64).reshape(-1, 2)
    q = np.trunc(SCALE * c + 0.5).astype(np.int64)                   # (numpy rounds the product, then the sum: no fused multiply-add)
    q = np.concatenate([q, q[:1]])
    return q[:, 0], q[:, 1]


def boundary_points(X, Y):
    """The lists u, v of rleFrPoly's first loop: every edge's points in order."""
    us, vs = [], []
    for j in range(len(X) - 1):
        xs, xe, ys, ye = int(X[j]), int(X[j + 1]), int(Y[j]), int(Y[j + 1])
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:                                      # C divides 0 by 0 here; the header gives the edge its one point
            us.append(np.array([xs], np.int64)); vs.append(np.array([ys], np.int64))
            continue
        s = np.float64(ye - ys) / np.float64(dx) if dx >= dy else np.float64(xe - xs) / np.float64(dy)
        d = np.arange(max(dx, dy) + 1, dtype=np.int64)
        t = (max(dx, dy) - d) if flip else d
        if dx >= dy:
            us.append(t + xs); vs.append(np.trunc(np.float64(ys) + s * t.astype(np.float64) + 0.5).astype(np.int64))
        else:
            vs.append(t + ys); us.append(np.trunc(np.float64(xs) + s * t.astype(np.float64) + 0.5).astype(np.int64))
    return np.concatenate(us), np.concatenate(vs)


def toggles(u, v, H, W):
    """rleFrPoly's second loop over j = 1 .. m - 1 (every pair at once, each with the C arithmetic in float64) -> the positions
    x H + y in pair order, H W among them when y clamps at H in the last column."""
    a, b = u[1:], u[:-1]
    differ = a != b
    xd = (np.minimum(a, b)[differ].astype(np.float64) + 0.5) / SCALE - 0.5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= W - 1)
    yd = (np.minimum(v[1:], v[:-1])[differ][keep].astype(np.float64) + 0.5) / SCALE - 0.5
    yd = np.ceil(np.where(yd < 0, 0.0, np.where(yd > H, np.float64(H), yd)))
    return xd[keep].astype(np.int64) * H + yd.astype(np.int64)


def toggle_counts(pos, H, W):
    """rleFrPoly's end: H W appended, sorted, differences, and the merge that drops a zero count with its neighbour -> COCO counts."""
    a = np.sort(np.append(np.asarray(pos, np.int64), H * W)).tolist()
    k, prev = len(a), 0
    for j in range(k):
        a[j], prev = a[j] - prev, a[j]
    b, j = [a[0]], 1
    while j < k:
        if a[j] > 0:
            b.append(a[j]); j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]; j += 1
    return np.asarray(b, np.int64)


def counts_mask(counts, H, W):
    """bool [H, W] of COCO counts: the 2nd, 4th, ... runs are foreground along p = x H + y (cut at H W, as rleDecode's caller sees)."""
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, counts)[:H * W]
    flat = np.concatenate([flat, np.zeros(H * W - flat.size, bool)])
    return flat.reshape(W, H).T.copy()


def parity_mask(pos, H, W):
    """Step 4 of the header: position p is foreground iff the toggles at positions <= p are odd in number."""
    hits = np.bincount(np.asarray(pos, np.int64), minlength=H * W + 1)[:H * W]
    return (np.cumsum(hits) % 2 == 1).reshape(W, H).T.copy()


def polygon_toggles(poly, H, W):
    return toggles(*boundary_points(*scaled_vertices(poly)), H, W)


def polygon_mask(poly, H, W):
    """bool [H, W] of one polygon through the counts, as rleFrPoly gives it."""
    return counts_mask(toggle_counts(polygon_toggles(poly, H, W), H, W), H, W)


def polygon_ok(poly, H, W):
    c = np.asarray(poly, np.float64).reshape(-1, 2)
    if c.shape[0] == 0 or not np.isfinite(c).all():
        return False
    return bool((c[:, 0] >= -MARGIN).all() and (c[:, 0] <= W + MARGIN).all() and (c[:, 1] >= -MARGIN).all() and (c[:, 1] <= H + MARGIN).all())


def decode(xy, poly_off, ann_poly_off, ann_image, ann_value, N, H, W):
    """(labels int32 [N, H, W], ann_area int64 [A]) of camo_poly_decode (offsets non-decreasing)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    labels = np.zeros((N, H, W), np.int32)
    A = len(ann_image)
    area = np.zeros(A, np.int64)
    for a in range(A):
        polys = [xy[poly_off[q]:poly_off[q + 1]] for q in range(ann_poly_off[a], ann_poly_off[a + 1])]
        if not 0 <= ann_image[a] < N or ann_value[a] < 1 or not all(polygon_ok(p, H, W) for p in polys):
            area[a] = -1
            continue
        union = np.zeros((H, W), bool)
        for p in polys:
            union |= polygon_mask(p, H, W)
        area[a] = union.sum()
        img = labels[ann_image[a]]
        img[union] = np.maximum(img[union], ann_value[a])
    return labels, area


def arrays(per_image):
    """[[(polygons, value), ...] per image], polygons a list of flat coordinate lists -> (xy [V, 2], poly_off, ann_poly_off,
    ann_image, ann_value) as camo_poly_decode takes them."""
    xy, poly_off, ann_poly_off, img, val = [], [0], [0], [], []
    for n, anns in enumerate(per_image):
        for polys, value in anns:
            for p in polys:
                c = np.asarray(p, np.float64).reshape(-1, 2)
                xy.append(c)
                poly_off.append(poly_off[-1] + len(c))
            ann_poly_off.append(len(poly_off) - 1)
            img.append(n); val.append(value)
    flat = np.concatenate(xy) if xy else np.zeros((0, 2), np.float64)
    return flat, np.asarray(poly_off, np.int32), np.asarray(ann_poly_off, np.int32), np.asarray(img, np.int32), np.asarray(val, np.int32)


def label_map(anns, H, W):
    """int32 [H, W] of one image's [(polygons, value)] list."""
    return decode(*arrays([anns]), 1, H, W)[0][0]


def contracted_mask(poly, H, W):
    """NOT the definition: the mask a kernel gives whose compiler contracted steps 1 and 2 into fused multiply-adds --
    fma(5, c, 0.5) and fma(s, t, a) + 0.5, the fused operation rounded once (exact rationals, then the nearest double).  The tests
    use it to show that their rounding cases tell such a kernel from a correct one."""
    c = np.asarray(poly, np.float64).reshape(-1, 2)
    q = [[int(float(5 * Fraction(float(v)) + Fraction(1, 2))) for v in p] for p in c]
    q.append(q[0])
    us, vs = [], []
    for (xs, ys), (xe, ye) in zip(q[:-1], q[1:]):
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:
            us.append(xs); vs.append(ys)
            continue
        n = max(dx, dy)
        s = float(np.float64(ye - ys) / np.float64(dx)) if dx >= dy else float(np.float64(xe - xs) / np.float64(dy))
        for d in range(n + 1):
            t = n - d if flip else d
            if dx >= dy:
                us.append(xs + t); vs.append(int(float(Fraction(s) * t + ys) + 0.5))
            else:
                vs.append(ys + t); us.append(int(float(Fraction(s) * t + xs) + 0.5))
    pos = toggles(np.asarray(us, np.int64), np.asarray(vs, np.int64), H, W)
    return counts_mask(toggle_counts(pos, H, W), H, W)
