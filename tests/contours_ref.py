"""include/camo_contours.h restated in numpy, SEQUENTIALLY: every crack of an image in index order, and from every
crack not yet seen the walk along the header's successor rule until it closes.  Deliberately not the pointer doubling the kernels
use.  The kernels are held to this file byte for byte."""
import numpy as np

HEADING = ((1, 0), (0, 1), (-1, 0), (0, -1))          # of side 0 top, 1 right, 2 bottom, 3 left: the pixel lies on the crack's right, y down
START = ((0, 0), (1, 0), (1, 1), (0, 1))              # the corner a side's crack starts at, as an offset from (x, y)


def _at(img, y, x):
    H, W = img.shape
    return int(img[y, x]) if 0 <= y < H and 0 <= x < W else 0      # everything outside the image is background


def is_crack(img, y, x, s):
    L = _at(img, y, x)
    dx, dy = HEADING[(s + 3) % 4]                      # the neighbour across side s: top (0, -1), right (1, 0), bottom (0, 1), left (-1, 0)
    return L > 0 and _at(img, y + dy, x + dx) != L


def crack_sides(img):
    """bool [H, W, 4]: ``is_crack`` of every side at once."""
    img = np.asarray(img, np.int64)
    pad = np.pad(img, 1)                                             # (background all round)
    across = np.stack([pad[:-2, 1:-1], pad[1:-1, 2:], pad[2:, 1:-1], pad[1:-1, :-2]], axis=-1)      # top, right, bottom, left
    return (img[..., None] > 0) & (across != img[..., None])


def successor(img, y, x, s, connectivity):
    """The crack after (pixel (y, x), side s): -> (y, x, s)."""
    L = _at(img, y, x)
    dx, dy = HEADING[s]
    by, bx = y + dy, x + dx                            # b: the pixel after p along the heading
    ay, ax = by - dx, bx + dy                          # a: the pixel to the left of b (left of (dx, dy) is (dy, -dx))
    a, b = _at(img, ay, ax) == L, _at(img, by, bx) == L
    if a and (b or connectivity == 8):
        return ay, ax, (s + 3) % 4
    if b:
        return by, bx, s
    return y, x, (s + 1) % 4


def trace_image(img, connectivity):
    """One image int32 [H, W] -> (E, rings) with rings a list of (label, first crack, [(x, y), ...] vertices, a2) in order of first crack."""
    H, W = img.shape
    cracks = np.flatnonzero(crack_sides(img)).tolist()               # (index 4 (y W + x) + s, increasing)
    seen, rings = set(), []
    for e in cracks:                                   # (increasing index: a ring is met at its first crack)
        if e in seen:
            continue
        y, x, s = (e // 4) // W, (e // 4) % W, e % 4
        verts, a2, walk = [], 0, []
        while True:
            walk.append((y, x, s))
            seen.add(4 * (y * W + x) + s)
            y, x, s = successor(img, y, x, s, connectivity)
            if 4 * (y * W + x) + s == e:
                break
        prev = walk[-1][2]                             # the first crack's predecessor closes the ring
        for (cy, cx, cs) in walk:
            x0, y0 = cx + START[cs][0], cy + START[cs][1]
            x1, y1 = x0 + HEADING[cs][0], y0 + HEADING[cs][1]
            a2 += x0 * y1 - x1 * y0
            if prev != cs:
                verts.append((x0, y0))
            prev = cs
        rings.append((int(img[e // 4 // W, (e // 4) % W]), e, verts, a2))
    return len(cracks), rings


def contours(labels, connectivity, C, R, V):
    """(rings int64 [N, R, 5], xy int32 [N, V, 2], counts int32 [N, 6]) of camo_contours."""
    labels = np.asarray(labels, np.int32)
    N = labels.shape[0]
    rings = np.zeros((N, R, 5), np.int64)
    xy = np.zeros((N, V, 2), np.int32)
    counts = np.zeros((N, 6), np.int32)
    for n in range(N):
        E, found = trace_image(labels[n], connectivity)
        if E > C:
            counts[n] = (E, 0, 0, 0, 0, 0)
            continue
        flat = [v for _, _, verts, _ in found for v in verts]
        off = 0
        for r, (label, e, verts, a2) in enumerate(found):
            if r < R:
                rings[n, r] = (label, e, off, len(verts), a2)
            off += len(verts)
        M, T = len(found), len(flat)
        if T:
            xy[n, :min(T, V)] = np.asarray(flat[:V], np.int32)
        counts[n] = (E, M, T, E, min(M, R), min(T, V))
    return rings, xy, counts


def polygons(found):
    """``trace_image``'s rings -> {id: (outer rings, hole rings)} as flat [x0, y0, x1, y1, ...] lists."""
    out = {}
    for label, _, verts, a2 in found:
        out.setdefault(label, ([], []))[0 if a2 > 0 else 1].append([c for v in verts for c in v])
    return out
