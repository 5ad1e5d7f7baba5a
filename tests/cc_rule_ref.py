"""The tiled union-find labelling of csrc/cc_inl.h, restated in numpy for a whole stack of small images at once and with the tile
side as a parameter: the run parents, exactly the unions the tile rule keeps and exactly the unions the border rule keeps, closed
by a plain minimum propagation.  No device, no library: this is where the rules are held to a flood fill (tests/test_cc_rule.py).

Two member pixels that touch are LINKED when their values are equal (``val`` None: always).  Names as in cc_inl.h."""
import numpy as np

BIG = np.iinfo(np.int64).max


def _at(a, dy, dx, fill=0):
    """a[..., y + dy, x + dx], ``fill`` outside the image."""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def links(member, val, same=np.equal):
    """-> left, up, nw, ne [M, H, W]: pixel p is linked to p - 1, p - W, p - W - 1, p - W + 1."""
    def link(dy, dx):
        both = member & _at(member, dy, dx)
        return both if val is None else both & same(val, _at(val, dy, dx))
    return link(0, -1), link(-1, 0), link(-1, -1), link(-1, 1)


def kept_unions(member, val, conn, T, same=np.equal):
    """-> (run_start [M, H, W] column of every pixel's run parent, {(dy, dx): [M, H, W] bool}): the unions that cc_run_parent,
    cc_tile_unions and cc_join_borders make."""
    member = np.asarray(member, bool)
    M, H, W = member.shape
    left, up, nw, ne = links(member, val, same)
    ty, tx = (np.arange(H) % T)[None, :, None], (np.arange(W) % T)[None, None, :]
    # cc_run_parent: the first pixel of the run in the tile row
    start = np.broadcast_to(np.arange(W), member.shape).copy()
    for x in range(1, W):
        if x % T:
            start[:, :, x] = np.where(left[:, :, x], start[:, :, x - 1], x)
    up_of_left, left_of_up = _at(up, 0, -1), _at(left, -1, 0)      # link(p-1, p-W-1), link(p-W, p-W-1)
    # cc_tile_unions (ty > 0; a diagonal neighbour inside the tile)
    by_left = (tx > 0) & left & up_of_left
    t_up = (ty > 0) & up & ~(by_left & left_of_up)
    t_nw = (ty > 0) & (tx > 0) & nw & ~up & ~by_left
    t_ne = (ty > 0) & (tx < T - 1) & ne & ~up
    # cc_join_borders
    nw_left, nw_up = up_of_left, left_of_up
    j_left = (tx == 0) & left & ~((ty != 0) & up & nw_up & nw_left)
    j_up = (ty == 0) & up & ~((tx != 0) & left & nw_left & nw_up)
    j_nw = ((ty == 0) | (tx == 0)) & nw & ~up & ~(left & nw_left)
    j_ne = ((ty == 0) | (tx == T - 1)) & ne & ~up
    unions = {(0, -1): j_left, (-1, 0): t_up | j_up}
    if conn == 8:
        unions[(-1, -1)] = t_nw | j_nw
        unions[(-1, 1)] = t_ne | j_ne
    return start, unions


def close(member, edges):
    """edges: [(cond [M, H, W], target flat index [M, H, W])] -> [M, H, W] the smallest index of every member's component, -1 elsewhere."""
    M, H, W = member.shape
    idx = np.broadcast_to(np.arange(H * W), (M, H * W))
    rows = np.broadcast_to(np.arange(M)[:, None], (M, H * W))
    L = np.where(member.reshape(M, -1), idx, BIG)
    pairs = []
    for cond, tgt in edges:
        cond = cond.reshape(M, -1)
        pairs.append((rows[cond], idx[cond], tgt.reshape(M, -1)[cond]))
    while True:
        before = L.copy()
        for r, p, t in pairs:
            m = np.minimum(L[r, p], L[r, t])
            np.minimum.at(L, (r, p), m)
            np.minimum.at(L, (r, t), m)
        if np.array_equal(L, before):
            break
    return np.where(member, L.reshape(M, H, W), -1)


def label(member, val, conn, T, same=np.equal):
    """The partition the device code computes: [M, H, W] smallest index of every member's component, -1 for a non-member."""
    member = np.asarray(member, bool)
    M, H, W = member.shape
    start, unions = kept_unions(member, val, conn, T, same)
    idx = np.broadcast_to(np.arange(H * W).reshape(H, W), member.shape)
    edges = [(member, idx - np.arange(W) + start)]
    edges += [(cond, idx + dy * W + dx) for (dy, dx), cond in unions.items()]
    return close(member, edges)


def flood(member, val, conn):
    """The same partition from scipy.ndimage.label, value by value (cross for 4, full structure for 8)."""
    from scipy import ndimage
    member = np.asarray(member, bool)
    M, H, W = member.shape
    s = np.zeros((3, 3, 3), int)      # (no link between the images of the stack)
    s[1] = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
    out = np.full(member.shape, -1, np.int64)
    idx = np.broadcast_to(np.arange(H * W).reshape(H, W), member.shape)
    for v in ([None] if val is None else np.unique(val[member])):
        sel = member if v is None else member & (val == v)
        lab, n = ndimage.label(sel, structure=s)
        first = np.full(n + 1, BIG)
        np.minimum.at(first, lab[sel], idx[sel])
        out[sel] = first[lab[sel]]
    return out


def all_links(member, val, conn, same):
    """The partition by every link, none left out and no tiles: the reference for a predicate that is no equivalence, where
    components are not regions of one value."""
    member = np.asarray(member, bool)
    M, H, W = member.shape
    idx = np.broadcast_to(np.arange(H * W).reshape(H, W), member.shape)
    offsets = [(0, -1), (-1, 0), (-1, -1), (-1, 1)][:2 if conn == 4 else 4]
    return close(member, [(c, idx + dy * W + dx) for (dy, dx), c in zip(offsets, links(member, val, same))])
