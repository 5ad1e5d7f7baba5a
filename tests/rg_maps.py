"""Label maps for the region-graph construction tests, in plain numpy: the shapes RO.voronoi_segments does not give (labels past
1024, label 0 in use, one-pixel regions, enclosure, stripes, a checkerboard, a label in two pieces, images narrower than the halo,
flat colours).  Every generator returns (image fp32 [H, W, 3] in [0, 1], seg int32 [H, W], canny bool [H, W]); images are uniform
noise unless said otherwise.  What each map is FOR is asserted on the CPU in test_rg_graph_shapes.py before any device is asked.

case(name) and oracle(name) are cached and never written to; check_against_oracle is the batch comparison with the project's bounds
(test_rg_batch.py and test_rg_graph_shapes.py share it)."""
import functools

import numpy as np

from oracle import rg_features_oracle as RO

CHUNK = 1024                       # labels a block of the rank / finalize / scan kernels takes per step
FLAT_A, FLAT_B = np.array([1.0, 0.0, 0.3], np.float32), np.array([0.0, 1.0, 0.7], np.float32)


def _noise(H, W, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, (H, W, 3)).astype(np.float32), rs.uniform(0, 1, (H, W)) > 0.85


def _yx(H, W):
    return np.meshgrid(np.arange(H), np.arange(W), indexing="ij")


def _pack(noise, seg):
    img, canny = noise
    assert img.shape[:2] == seg.shape == canny.shape and seg.dtype == np.int32
    return img, seg, canny


def perm64():
    """64 x 64, every pixel its own label 0 .. 4095 in a fixed random order."""
    seg = np.random.RandomState(0).permutation(4096).reshape(64, 64).astype(np.int32)
    return _pack(_noise(64, 64, 100), seg)


def blocks96():
    """96 x 96 in 2 x 2 blocks, label (y // 2) * 48 + x // 2: 2304 labels from 0."""
    yy, xx = _yx(96, 96)
    return _pack(_noise(96, 96, 101), ((yy // 2) * 48 + xx // 2).astype(np.int32))


SPARSE_FIXED = (0, 1023, 1024, 2047, 2048, 3071, 3072)      # label 0 and both sides of every chunk border
SPARSE_TOP = 3600                                           # labels stay below it: a label_bound between the labels and 4096 exists


def sparse_high():
    """64 x 48 Voronoi map of 40 regions, its labels 1 .. 40 sent into [0, SPARSE_TOP) by a fixed random injection that hits
    SPARSE_FIXED: a few labels in each chunk of 1024, most of every chunk empty."""
    seg = RO.voronoi_segments(64, 48, 40, 12)
    rest = np.setdiff1d(np.arange(SPARSE_TOP), SPARSE_FIXED)
    rs = np.random.RandomState(13)
    to = rs.permutation(np.concatenate([SPARSE_FIXED, rs.choice(rest, 40 - len(SPARSE_FIXED), replace=False)]))
    table = np.full(41, -1, np.int64)
    table[1:] = to
    return _pack(_noise(64, 48, 102), table[seg].astype(np.int32))


def rings():
    """48 x 48 concentric square rings of width 3, labels 1 .. 8 from the 6 x 6 centre outwards."""
    yy, xx = _yx(48, 48)
    d = np.maximum(np.abs(2 * yy - 47), np.abs(2 * xx - 47)) // 2           # 0 .. 23: Chebyshev distance from the centre
    return _pack(_noise(48, 48, 103), (1 + d // 3).astype(np.int32))


def stripes(transposed=False):
    """40 x 33 in one-pixel-wide vertical stripes cycling over labels 1 .. 5; transposed: 33 x 40 in horizontal stripes."""
    _, xx = _yx(40, 33)
    seg = (1 + xx % 5).astype(np.int32)
    if transposed:
        seg = np.ascontiguousarray(seg.T)
    return _pack(_noise(*seg.shape, 104 + transposed), seg)


def checker():
    """33 x 70 checkerboard of labels 1 and 2."""
    yy, xx = _yx(33, 70)
    return _pack(_noise(33, 70, 106), (1 + (xx + yy) % 2).astype(np.int32))


SPLIT_LABEL = 3


def split():
    """70 x 70 Voronoi map of 12 regions turned upside down, so that label 3 lies in the 32 x 32 tile at (32, 32); a 6 x 6 patch of
    the tile at (0, 0) is painted with label 3 as well."""
    seg = np.ascontiguousarray(RO.voronoi_segments(70, 70, 12, 14)[::-1])
    seg[4:10, 3:9] = SPLIT_LABEL
    return _pack(_noise(70, 70, 107), seg)


THIN_SHAPES = ((1, 1), (1, 70), (70, 1), (2, 2), (3, 35))


def thin(k):
    """Images narrower than the 2-pixel halo on one axis or both: THIN_SHAPES[k], with 1, 6, 5, 4 and 6 labels."""
    H, W = THIN_SHAPES[k]
    yy, xx = _yx(H, W)
    seg = [np.zeros((1, 1)), xx // 12, yy // 14 + 1, 2 * yy + xx, (xx // 6 + yy) % 6 + 1][k]
    return _pack(_noise(H, W, 108 + k), seg.astype(np.int32))


def flat(k):
    """k = 0: a saturated two-colour image whose regions are flat (every region of a 12-region map has one of two colours, no edge
    pixels).  k = 1: 64 x 64, labels 1 and 2 either side of a diagonal, every pixel the fp32 value 0.7 in all three channels."""
    if k == 0:
        seg = RO.voronoi_segments(64, 48, 12, 8)
        return np.where((seg % 2 == 0)[..., None], FLAT_A, FLAT_B).astype(np.float32), seg, np.zeros((64, 48), bool)
    yy, xx = _yx(64, 64)
    return np.full((64, 64, 3), 0.7, np.float32), (1 + (xx + yy >= 64)).astype(np.int32), _noise(64, 64, 113)[1]


CASES = {"perm64": perm64, "blocks96": blocks96, "sparse_high": sparse_high, "rings": rings, "stripes": stripes,
         "stripes_t": functools.partial(stripes, True), "checker": checker, "split": split,
         **{f"thin_{H}x{W}": functools.partial(thin, k) for k, (H, W) in enumerate(THIN_SHAPES)},
         "flat_two_colour": functools.partial(flat, 0), "flat_one_colour": functools.partial(flat, 1)}
FLAT_CASES = ("flat_two_colour", "flat_one_colour")


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, seg, canny) of CASES[name], read-only."""
    out = CASES[name]()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """RO.region_graph on case(name): (x, edge_index, edge_attr, region_map), read-only."""
    out = RO.region_graph(*case(name))
    for a in out:
        a.setflags(write=False)
    return out


def labels_per_chunk(seg):
    """Non-empty labels in [0, 1024), [1024, 2048), [2048, 3072), [3072, 4096)."""
    return np.bincount(np.unique(seg) // CHUNK, minlength=4).tolist()


def most_labels_in_a_tile(seg, tile=32):
    H, W = seg.shape
    return max(len(np.unique(seg[y:y + tile, x:x + tile])) for y in range(0, H, tile) for x in range(0, W, tile))


def most_distinct_neighbours(seg):
    """The largest number of distinct labels other than a pixel's own within L1 distance 2 of it."""
    H, W = seg.shape
    off = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if 0 < abs(dy) + abs(dx) <= 2]
    best = 0
    for y in range(H):
        for x in range(W):
            near = {int(seg[y + dy, x + dx]) for dy, dx in off if 0 <= y + dy < H and 0 <= x + dx < W}
            best = max(best, len(near - {int(seg[y, x])}))
    return best


def x_bound(x):
    """The project's bound on the 15 features against the oracle's x: 2e-6 x column scale (floor 1e-3) + 2e-6 |x|."""
    return 2e-6 * np.maximum(np.abs(x).max(0), 1e-3) + 2e-6 * np.abs(x)


def w_bound(ea):
    return 2e-5 * ea + 1e-9


def check_against_oracle(g, rm, want, what=""):
    """Every image's slice of the batch against (x, edge_index, edge_attr, region_map) of the oracle: the project's bounds."""
    no, eo = g.node_offsets, g.edge_offsets
    assert g.num_graphs == len(want) and len(no) == len(eo) == len(want) + 1 and no[0] == 0 and eo[0] == 0
    assert g.x.shape == (no[-1], 15) and g.edge_index.shape == (2, eo[-1]) and g.edge_attr.shape == (eo[-1], 1) and g.batch.shape == (no[-1],)
    gx, gei, gea, rm = g.x.cpu().numpy(), g.edge_index.cpu().numpy(), g.edge_attr.cpu().numpy()[:, 0], rm.cpu().numpy()
    worst_x, worst_w = 0.0, 0.0
    for k, (x, ei, ea, rmap) in enumerate(want):
        assert (rm[k, :len(rmap)] == rmap).all() and (rm[k, len(rmap):] == -1).all(), (what, k)
        assert no[k + 1] - no[k] == x.shape[0] and eo[k + 1] - eo[k] == ei.shape[1], (what, k, no, eo)
        assert (gei[:, eo[k]:eo[k + 1]] - no[k] == ei).all(), (what, k)                      # same order: sorted (i, j), each followed by its reverse
        xs = gx[no[k]:no[k + 1]]
        scale = np.maximum(np.abs(x).max(0), 1e-3)
        bound = 2e-6 * scale + 2e-6 * np.abs(x)
        worst_x = max(worst_x, float((np.abs(xs - x) / bound).max()))
        assert (np.abs(xs - x) <= bound).all(), (what, k, np.abs(xs - x).max(0) / scale)
        ws = gea[eo[k]:eo[k + 1]]
        if len(ea):
            worst_w = max(worst_w, float((np.abs(ws - ea) / (2e-5 * ea + 1e-9)).max()))
        assert (np.abs(ws - ea) <= 2e-5 * ea + 1e-9).all(), (what, k)
    counts = np.diff(no)
    assert (g.batch.cpu().numpy() == np.repeat(np.arange(len(want)), counts)).all()
    print(f"{what}: worst |x - oracle| / bound {worst_x:.3f}, worst |w - oracle| / bound {worst_w:.3f}")
    return worst_x, worst_w
