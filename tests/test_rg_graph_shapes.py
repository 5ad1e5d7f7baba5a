"""Region-graph construction (include/camo_rg_features.h, include/camo_rg_batch.h) off the Voronoi maps: labels at and past 1024,
batches past 64 and 256 images, pixels with 12 distinct neighbour labels, regions that are not convex cells, flat regions.

The maps are rg_maps.py's; what each one is FOR -- labels per chunk of 1024, more labels in a 32 x 32 tile than its hash table holds,
12 distinct neighbours, label 0 in use, a disconnected label -- is asserted on the CPU (test 1) before a device is asked.  Every
map goes through create_region_graph_from_segments and, as a batch of one, through create_region_graphs_from_segments, and both are
held to oracle/rg_features_oracle.py with the project's bounds (x within 2e-6 column scale + 2e-6 |x|, weights within 2e-5 w + 1e-9,
region_map and edge_index equal).  The one exception is derived, not measured: on the single-image path the std features of the
flat maps and of perm64's one-pixel regions are held to max(that bound, sqrt(CAMO_RG_VAR_BOUND_PER_PIXEL n)) for a region of n
pixels, the header's bound for double sums in arrival order; the batch path gives exactly 0 there, as its header promises.

Measured on the MI355X: see DESIGN.md, "Region-graph construction", the paragraph on the shapes of this file."""
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import rg_maps as M
from conftest import ROOT
from raw_calls import BUILDERS, execute
from oracle import rg_features_oracle as RO
from test_rg_batch import _build, _bytes, _mixed, _oracle

STD_COLS = [3, 4, 5, 7]                                     # std R, G, B, luma; 14 is the luma variance
EXACT_ZERO = M.FLAT_CASES + ("perm64",)                     # maps whose regions all have variance 0 in exact arithmetic


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_each_map_reaches_what_it_is_for():
    from camouflage_multimodal_amd import _lib
    per_chunk = {n: M.labels_per_chunk(M.case(n)[1]) for n in M.CASES}
    assert per_chunk["perm64"] == [1024, 1024, 1024, 1024] and per_chunk["blocks96"] == [1024, 1024, 256, 0]
    assert per_chunk["sparse_high"] == [14, 15, 6, 5]        # base carried across chunks that are mostly empty
    for n in M.CASES:
        img, seg, canny = M.case(n)
        assert img.dtype == np.float32 and seg.dtype == np.int32 and canny.dtype == bool and img.shape == seg.shape + (3,) == canny.shape + (3,)
        assert 0 <= img.min() and img.max() <= 1 and 0 <= seg.min() and seg.max() < _lib.RG_MAX_LABELS
        if n not in ("perm64", "blocks96", "sparse_high"):
            assert per_chunk[n][1:] == [0, 0, 0] and 1 <= per_chunk[n][0] <= 12, n
    # the adjacency rows: 128 and 72 words of 32 bits, the count kernel's second step of 64 words
    assert (M.case("perm64")[1].max() + 1 + 31) // 32 == 128 and (M.case("blocks96")[1].max() + 1 + 31) // 32 == 72
    assert M.most_labels_in_a_tile(M.case("perm64")[1]) == 1024 > _lib.RGB_TILE_SLOTS
    assert M.most_labels_in_a_tile(M.case("blocks96")[1]) == 256 > _lib.RGB_TILE_SLOTS
    assert M.most_distinct_neighbours(M.case("perm64")[1]) == 12
    for n in ("perm64", "blocks96", "sparse_high", "thin_1x1", "thin_1x70", "thin_2x2"):
        assert (M.case(n)[1] == 0).any(), n                   # label 0 in use
    seg = M.case("sparse_high")[1]
    assert set(M.SPARSE_FIXED) <= set(np.unique(seg).tolist()) and len(np.unique(seg)) == 40 and seg.max() < M.SPARSE_TOP
    seg = M.case("split")[1]
    assert ndimage.label(seg == M.SPLIT_LABEL)[1] == 2        # (4-connectivity; the pieces are 20 pixels apart)
    assert (seg[32:64, 32:64] == M.SPLIT_LABEL).sum() > 100 and (seg[:32, :32] == M.SPLIT_LABEL).sum() == 36
    seg = M.case("rings")[1]
    for lab in range(2, 8):                                   # every ring but the outermost is enclosed: its neighbours are lab - 1 inside, lab + 1 outside
        assert set(np.unique(ndimage.binary_dilation(seg == lab, np.ones((3, 3), bool)) * seg).tolist()) == {0, lab - 1, lab, lab + 1}
    for n in ("stripes", "stripes_t"):
        seg = M.case(n)[1]
        row = seg[0] if n == "stripes" else seg[:, 0]
        assert (row[:-2] != row[2:]).all() and (row[:-1] != row[1:]).all() and (row[:-5] == row[5:]).all()
        assert ndimage.label(seg == 1)[1] == 7               # 33 stripes over 5 labels
    seg = M.case("checker")[1]
    assert (seg[:, :-1] != seg[:, 1:]).all() and (seg[:-1] != seg[1:]).all() and set(np.unique(seg).tolist()) == {1, 2}
    assert [M.case(n)[1].shape for n in M.CASES if n.startswith("thin")] == list(M.THIN_SHAPES)
    assert [len(np.unique(M.case(n)[1])) for n in M.CASES if n.startswith("thin")] == [1, 6, 5, 4, 6]
    for n in M.FLAT_CASES:                                    # one colour per region
        img, seg, _ = M.case(n)
        assert all(len(np.unique(img[seg == lab], axis=0)) == 1 for lab in np.unique(seg)), n
    assert (M.case("flat_one_colour")[0] == np.float32(0.7)).all()


def test_oracle_sizes_on_the_large_maps():
    x, ei, ea, rmap = M.oracle("perm64")
    assert x.shape == (4096, 15) and ei.shape == (2, 32004) and (rmap == np.arange(4096)).all()
    assert (x[:, STD_COLS + [14]] == 0).all() and (x[:, 10] == np.float32(1 / 65536)).all()          # every region one pixel
    x, ei, ea, rmap = M.oracle("blocks96")
    assert x.shape == (2304, 15) and ei.shape == (2, 17860) and (rmap == np.arange(2304)).all()
    x, ei, ea, rmap = M.oracle("sparse_high")
    assert x.shape[0] == 40 and (rmap >= 0).sum() == 40 and len(rmap) == M.case("sparse_high")[1].max() + 1 > 3072


def test_variance_bound_is_the_headers():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_rg_features.h")).read()
    stated = float(re.search(r"#define CAMO_RG_VAR_BOUND_PER_PIXEL ([0-9.e+-]+)", hdr).group(1))
    assert stated == 9 * 2.0 ** -53 == _lib.RG_VAR_BOUND_PER_PIXEL
    # the derivation's own figure, 3 (n + 2) 2^-53, stays below it for every n >= 1; sequential double sums of a flat region obey it
    n = np.arange(1, 1 << 16)
    assert (3 * (n + 2) * 2.0 ** -53 <= stated * n).all()
    v = np.full(65536, np.float32(0.7), np.float64)
    s1, s2 = np.cumsum(v)[-1], np.cumsum(v * v)[-1]          # (cumsum adds one by one, in order)
    var = s2 * (1.0 / 65536) - (s1 * (1.0 / 65536)) ** 2
    print(f"sequential f64 sums of 65536 x fp32(0.7): variance {var:.3e}, bound {stated * 65536:.3e}")
    assert var != 0 and abs(var) <= stated * 65536


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _arrays(name):
    return tuple(np.array(a) for a in M.case(name))          # writable copies: the cached arrays are read-only


def _single(name, **kw):
    from camouflage_multimodal_amd import create_region_graph_from_segments
    return create_region_graph_from_segments(*_arrays(name), **kw)


def _batch_of_one(name, **kw):
    img, seg, canny = _arrays(name)
    return _build(img[None], seg[None], canny[None], **kw)


def _std_bound(name, want):
    """The header's bound on the single-image path's std features, per kept region: sqrt(CAMO_RG_VAR_BOUND_PER_PIXEL n)."""
    from camouflage_multimodal_amd import _lib
    n = np.bincount(M.case(name)[1].ravel(), minlength=len(want[3]))[want[3] >= 0]
    return np.sqrt(_lib.RG_VAR_BOUND_PER_PIXEL * n)


def _check_single(name, data, rm, want):
    """One image's graph of the single-image path against the oracle: the project's bounds, and on the maps of EXACT_ZERO the
    header's derived bound for the std features where it is the larger one (a rule on the reference alone)."""
    x, ei, ea, rmap = want
    assert (rm.cpu().numpy() == rmap).all(), name
    gx, ga = data.x.cpu().numpy(), data.edge_attr.cpu().numpy()
    assert gx.shape == x.shape and (data.edge_index.cpu().numpy() == ei).all(), name
    bound = M.x_bound(x)
    if name in EXACT_ZERO:
        bound[:, STD_COLS] = np.maximum(bound[:, STD_COLS], _std_bound(name, want)[:, None])
    worst_x = float((np.abs(gx - x) / bound).max())
    worst_w = float((np.abs(ga[:, 0] - ea) / M.w_bound(ea)).max()) if len(ea) else 0.0
    print(f"{name}, single image: worst |x - oracle| / bound {worst_x:.3f}, worst |w - oracle| / bound {worst_w:.3f}")
    assert (np.abs(gx - x) <= bound).all(), (name, (np.abs(gx - x) / bound).max(0))
    assert ga.shape == (len(ea), 1) and (np.abs(ga[:, 0] - ea) <= M.w_bound(ea)).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.CASES))
def test_single_image_path_matches_oracle(name):
    data, rm = _single(name)
    _check_single(name, data, rm, M.oracle(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.CASES))
def test_batch_path_matches_oracle(name):
    g, rm = _batch_of_one(name)
    M.check_against_oracle(g, rm, [M.oracle(name)], f"{name}, batch of one")
    if name in EXACT_ZERO:                                    # include/camo_rg_batch.h: a region of one flat colour has variance and std exactly 0
        assert (g.x[:, STD_COLS + [14]] == 0).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXACT_ZERO)
def test_flat_and_one_pixel_regions_on_the_single_image_path(name):
    """Means at the project's bound, std features within max(that bound, the header's sqrt(CAMO_RG_VAR_BOUND_PER_PIXEL n)); the
    measured maxima are printed before the assertions."""
    x, _, _, rmap = want = M.oracle(name)
    data, rm = _single(name)
    gx = data.x.cpu().numpy()
    assert gx.shape == x.shape and (rm.cpu().numpy() == rmap).all()
    derived = _std_bound(name, want)
    existing = M.x_bound(x)
    err = np.abs(gx - x)
    print(f"{name}, single image: largest std feature {np.abs(gx[:, STD_COLS]).max():.3e} (oracle {np.abs(x[:, STD_COLS]).max():.3e}), derived bound "
          f"{derived.min():.3e} .. {derived.max():.3e}, bound without it {existing[:, STD_COLS].min():.3e}; largest luma variance "
          f"{gx[:, 14].max():.3e}; worst mean error / bound {(err[:, [0, 1, 2, 6]] / existing[:, [0, 1, 2, 6]]).max():.3f}")
    assert (gx[:, STD_COLS + [14]] >= 0).all()
    assert (err[:, [0, 1, 2, 6]] <= existing[:, [0, 1, 2, 6]]).all()
    assert (err[:, STD_COLS] <= np.maximum(existing[:, STD_COLS], derived[:, None])).all()
    if name == "flat_two_colour":                             # the colours are 0, 0.3, 0.7 and 1: a mean of equal values is that value
        for row, lab in zip(gx, np.unique(M.case(name)[1])):
            assert np.allclose(row[:3], M.FLAT_A if lab % 2 == 0 else M.FLAT_B, rtol=0, atol=2e-6), lab


N_MANY = 300
ALONE = (0, 63, 64, 65, 255, 256, 299)                      # both sides of the emit kernel's stride of 64 and the prefix's stride of 256


@functools.lru_cache(maxsize=None)
def _many():
    """300 images of 8 x 8 in 2 x 2 blocks over 1 to 6 labels (from 0) drawn per image; every 37th holds one label and has no edges."""
    rs = np.random.RandomState(21)
    img = rs.uniform(0, 1, (N_MANY, 8, 8, 3)).astype(np.float32)
    canny = rs.uniform(0, 1, (N_MANY, 8, 8)) > 0.85
    seg = np.zeros((N_MANY, 8, 8), np.int32)
    for k in range(N_MANY):
        labels = 1 if k % 37 == 0 else rs.randint(1, 7)
        lab = rs.permutation(6)[:labels][rs.randint(0, labels, (4, 4))]
        if k in ALONE[1:]:                                    # the images that are also run alone have edges: two labels at least
            lab[0, :2] = (lab[0, 1] + 1) % 6, lab[0, 1]
        seg[k] = np.kron(lab, np.ones((2, 2), np.int32))
    want = [RO.region_graph(img[k], seg[k], canny[k]) for k in range(N_MANY)]
    return img, seg, canny, want


@pytest.mark.gpu
def test_many_images_match_oracle_and_their_single_runs():
    img, seg, canny, want = _many()
    nodes, edges = [w[0].shape[0] for w in want], [w[1].shape[1] for w in want]
    assert all(edges[k] == 0 and nodes[k] == 1 for k in range(0, N_MANY, 37)) and sorted(set(nodes)) == [1, 2, 3, 4, 5, 6]
    assert all(edges[k] > 0 for k in ALONE[1:]) and len(np.unique(seg)) == 6
    g, rm = _build(img, seg, canny, label_bound=6)
    assert g.node_offsets == [0] + np.cumsum(nodes).tolist() and g.edge_offsets == [0] + np.cumsum(edges).tolist()
    assert (g.batch.cpu().numpy() == np.repeat(np.arange(N_MANY), nodes)).all()
    M.check_against_oracle(g, rm, want, f"{N_MANY} images of 8 x 8")
    no, eo = g.node_offsets, g.edge_offsets
    for k in ALONE:
        g1, rm1 = _build(img[k:k + 1], seg[k:k + 1], canny[k:k + 1], label_bound=6)
        assert g1.node_offsets == [0, nodes[k]] and g1.edge_offsets == [0, edges[k]], k
        assert g1.x.cpu().numpy().tobytes() == g.x[no[k]:no[k + 1]].cpu().numpy().tobytes(), k
        assert g1.edge_attr.cpu().numpy().tobytes() == g.edge_attr[eo[k]:eo[k + 1]].cpu().numpy().tobytes(), k
        assert g1.edge_index.cpu().numpy().tobytes() == (g.edge_index[:, eo[k]:eo[k + 1]] - no[k]).cpu().contiguous().numpy().tobytes(), k
        assert rm1.cpu().numpy().tobytes() == rm[k:k + 1].cpu().numpy().tobytes(), k
        assert (g1.batch.cpu() == 0).all() and (g.batch[no[k]:no[k + 1]].cpu() == k).all(), k


def _same_but_for_the_bound(tight, wide, what):
    (g, rm), (g2, rm2) = tight, wide
    assert _bytes(g, rm)[:4] == _bytes(g2, rm2)[:4] and _bytes(g, rm)[5:] == _bytes(g2, rm2)[5:], what       # x, edge_index, edge_attr, batch; offsets
    lb = rm.shape[1]
    assert rm2.shape[1] > lb and (rm2[:, :lb].cpu() == rm.cpu()).all() and (rm2[:, lb:].cpu() == -1).all(), what


@pytest.mark.gpu
def test_a_label_bound_above_the_labels_changes_nothing():
    img, seg, canny = _mixed()
    tight = _build(img, seg, canny, label_bound=41)
    M.check_against_oracle(*tight, _oracle("mixed"), "mixed batch, label_bound 41")
    _same_but_for_the_bound(tight, _build(img, seg, canny, label_bound=4096), "mixed, 4096")
    top = int(M.case("sparse_high")[1].max()) + 1
    assert 3073 <= top < 4000
    tight = _batch_of_one("sparse_high", label_bound=top)
    M.check_against_oracle(*tight, [M.oracle("sparse_high")], f"sparse_high, label_bound {top}")
    for lb in (top + 1, 4000, 4096):
        _same_but_for_the_bound(tight, _batch_of_one("sparse_high", label_bound=lb), f"sparse_high, {lb}")


@functools.lru_cache(maxsize=None)
def _production():
    """blocks96 with its first 1076 labels kept and the rest merged into label 0: labels 1024 .. 1075 in use under
    slic_label_bound(256, 256, 500) = 1076, the bound every 256 x 256 detector, fine-tuning and predict_batch call passes."""
    img, seg, canny = _arrays("blocks96")
    seg[seg >= 1076] = 0
    return img, seg, canny, RO.region_graph(img, seg, canny)


@pytest.mark.gpu
def test_the_production_label_bound_with_its_second_chunk_in_use():
    from camouflage_multimodal_amd import slic_label_bound
    img, seg, canny, want = _production()
    assert slic_label_bound(256, 256, 500) == 1076 and M.labels_per_chunk(seg) == [1024, 52, 0, 0] and want[0].shape[0] == 1076
    assert ndimage.label(seg == 0)[1] == 2                    # label 0: its own block and everything below the kept rows
    g, rm = _build(img[None], seg[None], canny[None], label_bound=1076)
    M.check_against_oracle(g, rm, [want], "blocks96 under label_bound 1076")
    from camouflage_multimodal_amd import create_region_graph_from_segments
    data, rm1 = create_region_graph_from_segments(img, seg, canny)
    _check_single("blocks96 under 1076 labels", data, rm1, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["perm64", "split"])
def test_two_batch_calls_give_the_same_bytes(name):
    assert _bytes(*_batch_of_one(name)) == _bytes(*_batch_of_one(name))


FILL = 0x7F                                                 # the byte every output and the workspace hold on entry


def _sentinel_inputs():
    img, seg, canny = _arrays("perm64")
    return img, seg, canny.astype(np.uint8), M.oracle("perm64")


def _edges_written(got, cap, want):
    """Columns below the capacity (pairs are written whole, so below the even part of it) hold the oracle's edges; nothing else is written."""
    _, wei, wea, _ = want
    ei, ea = got["edge_index"], got["edge_attr"]
    done = min(cap - cap % 2, wei.shape[1])
    assert (ei[:, :done] == wei[:, :done]).all()
    assert (np.abs(ea[:done] - wea[:done]) <= M.w_bound(wea[:done])).all()
    assert (np.ascontiguousarray(ei[:, done:]).view(np.uint8) == FILL).all() and (ea[done:].view(np.uint8) == FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("short", [0, 2, None])
def test_single_image_abi_writes_inside_its_buffers(short):
    """camo_rg_region_graph on perm64 (4096 labels, 32004 directed edges) with every output and the workspace between guards
    (tests/guarded.py) and filled with 0x7F, at an edge capacity of exactly the need, the need - 2, and 2: guards intact, nothing at
    or past the capacity, counts still the need."""
    img, seg, canny, want = _sentinel_inputs()
    need_e, n = want[1].shape[1], 4096
    cap = 2 if short is None else need_e - short
    got = execute(BUILDERS["camo_rg_region_graph"](img, seg, canny, n, cap), FILL)
    assert got["counts"].tolist() == [n, need_e]
    assert (got["region_map"] == want[3]).all()
    _edges_written(got, cap, want)


@pytest.mark.gpu
@pytest.mark.parametrize("short", [0, 2, None])
def test_batch_abi_writes_inside_its_buffers(short):
    """camo_rg_region_graph_batch likewise, N = 1 and label_bound = node_capacity = 4096."""
    img, seg, canny, want = _sentinel_inputs()
    need_e, n = want[1].shape[1], 4096
    cap = 2 if short is None else need_e - short
    got = execute(BUILDERS["camo_rg_region_graph_batch"](img[None], seg[None], canny[None], n, cap), FILL)
    assert got["status"].tolist() == [0, need_e] and got["node_off"].tolist() == [0, n] and got["edge_off"].tolist() == [0, need_e]
    assert (got["region_map"][0] == want[3]).all() and (got["batch"] == 0).all()
    _edges_written(got, cap, want)
