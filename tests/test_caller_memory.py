"""The image-pipeline entry points on memory they did not clear.

Every header under include/ says that the contents of a workspace and of an output array on entry are unspecified.  The modules' own
tests take both from torch.empty, which in a fresh process is mostly zero: a clear that is missing, covers the wrong extent or is
skipped for one mode passes them, and so does a carve a few elements short of what the kernels index.  Here every C entry point that
takes a workspace, or clears and accumulates into a caller array, is called through ctypes with the workspace of exactly
``*_workspace_bytes`` bytes and every input and output in a guarded tensor of its own, in three variants (the harness -- ``Call``,
``execute`` and one builder of a Call per entry point -- is tests/raw_calls.py on tests/guarded.py, shared with the modules' own tests;
this file keeps the cases):

  clean   every byte of the workspace and of the outputs is 0.  Held to the module's reference exactly as the module's own test
          holds it: integers bytewise, floats with that test's bound, magnitudes from the reference.  No tolerance is new here.
  0xFF    every byte is 0xFF: each int is -1, each float and double a NaN.
  stale   the same buffers after two other calls of the same entry point: a busier input of the same shape (a salted or
          checkerboard map, more ids, more runs), then the case's input with H and W exchanged -- the same pixel count, so every
          stale index is below the arrays' lengths, but tiles, chunks and segments lie elsewhere.  Where the exchanged shape asks for
          a larger workspace the buffer is that large, the part past the case's own size is refilled with 0xFF before the case's
          call, which is told its own size, and that part must come back untouched.

Two rules hold a dirty variant to the clean one (``bytewise`` of each entry, named in its docstring):
  BYTEWISE    the module's own test already asserts that two calls give the same bytes (integer sums, fixed-order arithmetic): the
              declared outputs of 0xFF and stale are byte-equal to clean's.
  REFERENCE   where it does not (camo_rg_region_graph sums doubles by atomics in arrival order): the dirty variants are held to
              the reference with the same bound as clean.
Every variant is held to the reference as well, so an element the header declares written either equals the reference or, for a
float, lies within its bound of it -- a sentinel NaN left in place fails every bound.  Elements a header declares NOT written
(x rows past the regions kept, edge columns past the edges found) are left out of both comparisons and of nothing else.

Four calls with per-pixel workspace pieces run once more at a pixel count one past a multiple of 256, where a carve one element
short moves the pieces behind it (the note in front of that test).  The last part runs the clears that go over a capped grid with a
stride loop past their caps, on 0xFF memory, against the numpy references bytewise: sizes the modules' own cases never reach, so the
stride was never taken."""
import functools
from fractions import Fraction as F
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import canny_ref as CR
import guided_ref as GR
import inst_match_ref as IMR
import instances_ref as IR
import rg_detect_ref as DR
import rg_maps as M
import rg_targets_ref as TG
import rle_ref as RR
import seg_measures_ref as SR
import slic_ref as SL
import test_canny as TC
import test_guided as TGD
import test_inst_match as TM
import test_instances as TI
import test_rg_graph_shapes as TGS
import test_rg_targets as TT
import test_rle as TR
import test_seg_measures as TS
import test_slic as TSL
from oracle import rg_features_oracle as RO
from raw_calls import BUILDERS, execute, same_bytes as _same_bytes

N3, H3, W3 = 3, 70, 133             # the free shape: more than one tile each way, a multiple of no tile or chunk, image 1 at an odd byte offset
VARIANTS = ("clean", "0xFF", "stale")


def _t(a):
    """H and W exchanged: [N, H, W, ...] -> [N, W, H, ...]."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose((0, 2, 1) + tuple(range(3, a.ndim))))


class Entry:
    """An entry point: build(variant) -> Call for "case", "busy" and "swapped"; check(got) holds the case's outputs to the
    reference; declared(got) -> the arrays (or their parts) the header declares written, which BYTEWISE compares."""
    bytewise = True

    def declared(self, got):
        return got

    def run(self, variant):
        case = self.build("case")
        if variant == "clean":
            return execute(case, 0x00)
        if variant == "0xFF":
            return execute(case, 0xFF)
        return execute(case, 0xFF, before=(self.build("busy"), self.build("swapped")))


# ---- Canny ------------------------------------------------------------------------------------------------------------------

class Canny(Entry):
    """camo_canny on test_canny's "3x96x80" (its seeds make the end-to-end criterion decidable; the shape is theirs): gradients
    within GRAD_BOUND of float64, decisions exact on the device's own gradients, the end-to-end criterion.  BYTEWISE:
    test_batch_equals_singles compares the bytes of separate calls."""
    name = "3x96x80"

    def build(self, variant):
        img = TC.CASES[self.name]
        if variant == "busy":
            img = np.random.RandomState(1).uniform(0, 1, img.shape).astype(np.float32)
        if variant == "swapped":
            img = _t(img)
        return BUILDERS["camo_canny"](img, 2.0, 0.1, 0.2)

    def check(self, got):
        e, g = got["edges"], got["grad"]
        assert set(np.unique(e).tolist()) <= {0, 1}
        for k in range(len(e)):
            g64 = TC._ref64(self.name)[k][1]
            err = max(float(np.abs(g64[c] - g[k, c]).max()) for c in range(3))
            assert err <= TC.GRAD_BOUND, (k, err)
            assert ((e[k] > 0) == CR.decide(g[k, 0], g[k, 1], g[k, 2], 0.1, 0.2)).all(), k
            TC._end_to_end(self.name, k, e[k] > 0, g[k])


def _class_maps(variant, shape=(N3, H3, W3)):
    u = np.random.RandomState(2).uniform(0, 1, shape)
    if variant == "busy":
        return (u < 0.9).astype(np.uint8) + (u < 0.01)
    cls = (u < 0.42).astype(np.uint8) + (u < 0.004)          # weak near the 8-connected percolation threshold, few strong
    return _t(cls) if variant == "swapped" else cls


class Hysteresis(Entry):
    """camo_canny_hysteresis on random class maps as test_hysteresis_on_random_class_maps draws them, against canny_ref.hysteresis
    exactly.  BYTEWISE: that test asserts two calls give the same bytes."""

    def __init__(self, shape=(N3, H3, W3)):
        self.shape = shape

    def build(self, variant):
        return BUILDERS["camo_canny_hysteresis"](_class_maps(variant, self.shape))

    @functools.lru_cache(maxsize=None)
    def _want(self):
        want = np.stack([CR.hysteresis(c) for c in _class_maps("case", self.shape)])
        assert 0 < want.sum() < (_class_maps("case", self.shape) > 0).sum()
        return want

    def check(self, got):
        e = got["edges"]
        assert set(np.unique(e).tolist()) <= {0, 1} and ((e > 0) == self._want()).all(), int(((e > 0) != self._want()).sum())


# ---- SLIC -------------------------------------------------------------------------------------------------------------------

class Slic(Entry):
    """camo_slic on slic_ref's "33x70" (its seeds keep every margin clear; the shape is theirs) against the float64 labels, as
    test_end_to_end_equals_float64.  BYTEWISE: test_whole_call_equals_its_stages_and_a_batch_its_images compares bytes across calls."""
    name = "33x70"

    def build(self, variant):
        img, n = TSL.CASES[self.name]
        if variant == "busy":
            img = np.random.RandomState(3).uniform(0, 1, img.shape).astype(np.float32)
        if variant == "swapped":
            img = _t(img)
        return BUILDERS["camo_slic"](img, n, 10.0, 1.0)

    def check(self, got):
        for k in range(len(got["labels"])):
            want, over = TSL._ref_labels(self.name, k)
            assert (got["labels"][k] == want).all(), (k, int((got["labels"][k] != want).sum()))
            assert got["counts"][k].tolist() == [want.max() + 1, over]


def _salted_maps(variant, shape=(N3, H3, W3)):
    rs = np.random.RandomState(4)
    if variant == "busy":
        return rs.randint(0, 3, shape).astype(np.int32)
    maps = np.stack([RO.voronoi_segments(shape[1], shape[2], 30, 4 + 7 * i) for i in range(shape[0])]).astype(np.int32)
    salt = rs.uniform(0, 1, maps.shape) < 0.02
    maps[salt] = rs.randint(0, 30, int(salt.sum()))
    return _t(maps) if variant == "swapped" else maps


class SlicConnect(Entry):
    """camo_slic_connect on salted Voronoi maps as test_connect_on_salted_voronoi_maps draws them, min_size 6, against
    slic_ref.connect exactly.  BYTEWISE: _check_connect asserts two calls give the same bytes."""

    def __init__(self, shape=(N3, H3, W3)):
        self.shape = shape

    def build(self, variant):
        return BUILDERS["camo_slic_connect"](_salted_maps(variant, self.shape), 6, 10 ** 6)

    @functools.lru_cache(maxsize=None)
    def _want(self):
        return [SL.connect(seg, 6, 10 ** 6) for seg in _salted_maps("case", self.shape)]

    def check(self, got):
        assert got["labels"].max() >= 10
        for k, (want, over) in enumerate(self._want()):
            assert (got["labels"][k] == want).all(), (k, int((got["labels"][k] != want).sum()))
            assert got["counts"][k].tolist() == [want.max() + 1, over]


class SlicUpdate(Entry):
    """camo_slic_update on the fifth iteration of slic_ref's "33x70", two centroids left without a pixel, as
    test_update_against_float64_means: bit for bit the float32 restatement, and within that test's bound of the float64 means.
    The dirty array is ``sums``, which the header calls scratch: any content on entry, nothing promised on exit, so it is guarded
    and left out of the comparison; ``centroids`` is in-out and holds the centroids on entry.  BYTEWISE: that test asserts two
    calls give the same bytes."""
    name = "33x70"

    @functools.lru_cache(maxsize=None)
    def _arrays(self, variant):
        N = len(TSL.CASES[self.name][0])
        lab = np.stack([TSL._ref(self.name, k)[0] for k in range(N)]).astype(np.float32)
        near = np.stack([TSL._ref(self.name, k)[1][4]["near"] for k in range(N)]).astype(np.int32)
        cent = np.stack([TSL._ref(self.name, k)[1][4]["cent"] for k in range(N)]).astype(np.float32)
        K = cent.shape[1]
        near[near == 1] = 0
        near[near == K - 2] = K - 1
        if variant == "busy":                                   # every centroid takes pixels from every tile
            near = np.random.RandomState(5).randint(0, K, near.shape).astype(np.int32)
        if variant == "swapped":
            lab, near = _t(lab), _t(near)
        return lab, near, cent

    def build(self, variant):
        return BUILDERS["camo_slic_update"](*self._arrays(variant))

    def declared(self, got):
        return {"centroids": got["centroids"]}

    def check(self, got):
        lab, near, cent = self._arrays("case")
        a, K = got["centroids"], cent.shape[1]
        for k in range(len(a)):
            assert a[k, 1].tobytes() == cent[k, 1].tobytes() and a[k, K - 2].tobytes() == cent[k, K - 2].tobytes()
            want = SL.update(lab[k].astype(np.float64), near[k], cent[k].astype(np.float64), np.float64)
            bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -40
            bound[:, 2:] += 2.0 ** -25
            assert (np.abs(a[k].astype(np.float64) - want) <= bound).all(), k
            assert a[k].tobytes() == SL.update(lab[k], near[k], cent[k], np.float32).tobytes(), k


# ---- region graphs and node targets ----------------------------------------------------------------------------------------

def _graph_inputs(variant, regions=40):
    """(images fp32 [N, H, W, 3], segments int32 [N, H, W], canny uint8 [N, H, W]): Voronoi maps, labels 1 .. regions."""
    rs = np.random.RandomState(6)
    img = rs.uniform(0, 1, (N3, H3, W3, 3)).astype(np.float32)
    canny = (rs.uniform(0, 1, (N3, H3, W3)) > 0.85).astype(np.uint8)
    seg = np.stack([RO.voronoi_segments(H3, W3, regions, 20 + i) for i in range(N3)]).astype(np.int32)
    assert seg.min() >= 1 and seg.max() == regions
    if variant == "busy":                                       # 2 x 2 blocks over all the labels, 0 included: far more adjacencies
        yy, xx = np.mgrid[0:H3, 0:W3]
        seg = np.broadcast_to(((yy // 2 * 67 + xx // 2) % (regions + 1)).astype(np.int32), seg.shape).copy()
        canny = 1 - canny
    if variant == "swapped":
        img, seg, canny = _t(img), _t(seg), _t(canny)
    return img, seg, canny


@functools.lru_cache(maxsize=None)
def _graph_oracle(k):
    img, seg, canny = _graph_inputs("case")
    return RO.region_graph(img[k], seg[k], canny[k] > 0)


def _check_single_graph(got, want, std_floor=None):
    """One image's graph of camo_rg_region_graph against the oracle with the project's bounds, as test_rg_graph_shapes._check_single."""
    x, ei, ea, rmap = want
    assert got["counts"].tolist() == [x.shape[0], ei.shape[1]]
    assert (got["region_map"] == rmap).all()
    bound = M.x_bound(x)
    if std_floor is not None:
        bound[:, TGS.STD_COLS] = np.maximum(bound[:, TGS.STD_COLS], std_floor[:, None])
    gx = got["x"][:x.shape[0]]
    assert (np.abs(gx - x) <= bound).all(), (np.abs(gx - x) / bound).max(0)
    assert (got["edge_index"] == ei).all()
    assert (np.abs(got["edge_attr"] - ea) <= M.w_bound(ea)).all()


class RegionGraph(Entry):
    """camo_rg_region_graph on image 1 of the free shape (it starts at an odd byte offset of the canny batch) against the oracle with
    the project's bounds, the edge capacity exactly the need.  REFERENCE: the per-region sums are doubles added by atomics in arrival
    order, so two calls need not give the same bytes and the module's tests do not ask it; every variant is held to the oracle.
    x rows past counts[0] are declared invalid and are not compared."""
    bytewise = False

    def build(self, variant):
        img, seg, canny = _graph_inputs(variant)
        return BUILDERS["camo_rg_region_graph"](img[1], seg[1], canny[1], 41, _graph_oracle(1)[1].shape[1])

    def check(self, got):
        _check_single_graph(got, _graph_oracle(1))


def _declared_batch_graph(got):
    n, e = int(got["node_off"][-1]), int(got["edge_off"][-1])
    return {"x": got["x"][:n], "region_map": got["region_map"], "edge_index": got["edge_index"][:, :e], "edge_attr": got["edge_attr"][:e],
            "node_off": got["node_off"], "edge_off": got["edge_off"], "batch": got["batch"][:n], "status": got["status"]}


def _check_batch_graph(got, want, what):
    N = len(want)
    d = _declared_batch_graph(got)
    assert d["status"].tolist() == [0, sum(w[1].shape[1] for w in want)] and d["node_off"][0] == 0 and d["edge_off"][0] == 0
    g = SimpleNamespace(num_graphs=N, node_offsets=d["node_off"].tolist(), edge_offsets=d["edge_off"].tolist(), x=torch.from_numpy(d["x"]),
                        edge_index=torch.from_numpy(d["edge_index"]), edge_attr=torch.from_numpy(d["edge_attr"][:, None]), batch=torch.from_numpy(d["batch"]))
    assert g.edge_offsets[-1] == got["edge_index"].shape[1]
    M.check_against_oracle(g, torch.from_numpy(d["region_map"]), want, what)


class RegionGraphBatch(Entry):
    """camo_rg_region_graph_batch on the free shape against the oracle image by image (rg_maps.check_against_oracle), the edge capacity
    exactly the need.  BYTEWISE: test_two_batch_calls_give_the_same_bytes.  x and batch rows past node_off[N] are declared invalid and are
    not compared."""

    def build(self, variant):
        img, seg, canny = _graph_inputs(variant)
        return BUILDERS["camo_rg_region_graph_batch"](img, seg, canny, 41, sum(_graph_oracle(k)[1].shape[1] for k in range(N3)))

    def declared(self, got):
        return _declared_batch_graph(got)

    def check(self, got):
        _check_batch_graph(got, [_graph_oracle(k) for k in range(N3)], "70 x 133 batch")


class NodeTargets(Entry):
    """camo_rg_node_targets on the free shape, all three masks given, band 100 and three edge pixels, against rg_targets_ref exactly:
    ``counts`` is the dirty accumulator (the call takes no workspace).  BYTEWISE:
    test_a_batch_is_its_images_one_by_one_and_two_calls_give_the_same_bytes."""

    @functools.lru_cache(maxsize=None)
    def _arrays(self, variant):
        _, seg, _ = _graph_inputs(variant)
        rmap, off = TG.compact_region_map(_graph_inputs("case")[1], 41)
        rs = np.random.RandomState(7)
        gt, inst, edge = TT._blobs(rs, N3, H3, W3), TT._blobs(rs, N3, H3, W3), TT._blobs(rs, N3, H3, W3, k=6)
        if variant == "busy":
            gt, inst, edge = 255 - gt, 255 - inst, 255 - edge
        if variant == "swapped":
            gt, inst, edge = _t(gt), _t(inst), _t(edge)
        return seg, rmap, off, gt, inst, edge

    def build(self, variant):
        arrays = self._arrays(variant)
        return BUILDERS["camo_rg_node_targets"](*arrays, int(arrays[2][-1]), 100, 3)

    def check(self, got):
        seg, rmap, off, gt, inst, edge = self._arrays("case")
        want = TG.node_targets(seg, rmap, off, gt, inst, edge, 100, 3)
        assert want[3][:, 0].sum() == N3 * H3 * W3 and {0, 1} <= set(want[0].tolist()) and 0 < want[3][:, 3].sum()
        _same_bytes(got, dict(zip(("mask_t", "inst_t", "edge_t", "counts"), want)), "node targets")


# ---- instances, matching, run lengths --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _instance_maps(variant, shape=(N3, H3, W3)):
    """pred fp32 [3, 70, 133]: test_instances' serpentine at this shape, its nested rings with an island, a ring with a gap and blobs of
    4 and 6 pixels, and noise at density 0.6.  Busy: a checkerboard, every pixel a component at connectivity 4.  Any other shape:
    noise at density 0.55 in every image, which has small components and holes."""
    if shape != (N3, H3, W3):
        assert variant == "case"
        m = np.random.RandomState(15).uniform(0, 1, shape) < 0.55
        pred = np.stack([TI._values(m[i], 40 + i) for i in range(shape[0])])
        pred.setflags(write=False)
        return pred
    m = np.zeros((N3, H3, W3), bool)
    m[0, 0::2] = True
    for i, r in enumerate(range(1, H3 - 1, 2)):
        m[0, r, W3 - 1 if i % 2 == 0 else 0] = True
    TI._ring(m[1], 4, 6, 60, 90)
    TI._ring(m[1], 14, 20, 50, 76)
    m[1, 30:35, 40:50] = True
    TI._ring(m[1], 10, 100, 40, 130)
    m[1, 10, 100] = False
    m[1, 64:66, 2:4] = True
    m[1, 66:68, 10:13] = True
    m[2] = np.random.RandomState(8).uniform(0, 1, (H3, W3)) < 0.6
    if variant == "busy":
        yy, xx = np.mgrid[0:H3, 0:W3]
        m[:] = (yy + xx) % 2 == 0
    pred = np.stack([TI._values(m[i], 30 + i) for i in range(N3)])
    pred = _t(pred) if variant == "swapped" else pred
    pred.setflags(write=False)
    return pred


class Instances(Entry):
    """camo_instances at one of its four modes (connectivity 4 / 8 x fill_holes off / on: the clears of area[], border[] and misc[]
    differ by mode), min_area 5, 64 table rows, against instances_ref bytewise.  BYTEWISE:
    test_a_batch_is_its_images_and_two_calls_are_the_same_bytes."""

    def __init__(self, connectivity, fill, shape=(N3, H3, W3)):
        self.connectivity, self.fill, self.shape = connectivity, fill, shape

    def build(self, variant):
        return BUILDERS["camo_instances"](_instance_maps(variant, self.shape), 0.5, self.connectivity, 5, self.fill, 64)

    def check(self, got):
        want = _instances_ref(self.connectivity, self.fill, self.shape)
        assert want[3][:, 0].min() >= 1 and want[3][:, 1].sum() >= 1 and (not self.fill or want[3][:, 2].sum() >= 1)
        TI._same([got[k] for k in ("labels", "clean", "table", "counts")], want, f"connectivity {self.connectivity}, fill {self.fill}")


@functools.lru_cache(maxsize=None)
def _instances_ref(connectivity, fill, shape=(N3, H3, W3)):
    return IR.instances(_instance_maps("case", shape), 0.5, connectivity, 5, fill, 64)


class InstMatch(Entry):
    """camo_inst_match on test_inst_match's "batch" (five images of 37 x 29, seven ids, a score table, the COCO thresholds) against
    inst_match_ref bytewise.  BYTEWISE: test_a_batch_is_its_images_and_two_calls_are_the_same_bytes."""

    def build(self, variant):
        pred, gt, P, G, table, thr = TM._case("batch")
        if variant == "busy":                                   # every pixel an id of its own draw: every pair of ids occurs
            rs = np.random.RandomState(9)
            pred, gt = rs.randint(0, P + 1, pred.shape).astype(np.int32), rs.randint(0, G + 1, gt.shape).astype(np.int32)
        if variant == "swapped":
            pred, gt = _t(pred), _t(gt)
        return BUILDERS["camo_inst_match"](pred, gt, P, G, table, thr)

    def check(self, got):
        _same_bytes(got, TM._ref("batch"), "batch")


class RleRuns(Entry):
    """camo_rle_runs on test_rle's "batch" (five images of 70 x 33) against rle_ref bytewise; the busy call is a checkerboard, a run
    at every pixel and far more than the capacity.  BYTEWISE: test_a_batch_is_its_images_and_two_calls_are_the_same_bytes."""

    def build(self, variant):
        labels, R_ = TR._case("batch")
        if variant == "busy":
            _, yy, xx = np.mgrid[0:labels.shape[0], 0:labels.shape[1], 0:labels.shape[2]]
            labels = ((xx + yy) % 2 * 9).astype(np.int32)
        if variant == "swapped":
            labels = _t(labels)
        return BUILDERS["camo_rle_runs"](labels, R_)

    def check(self, got):
        labels, R_ = TR._case("batch")
        _same_bytes(got, RR.runs_batch(labels, R_), "batch")


@functools.lru_cache(maxsize=None)
def _annotations(variant):
    """Forty rectangle annotations over three images as test_decode_of_many_annotations_over_three_images draws them (some empty); busy:
    the same forty as checkerboards inside their rectangles, a run at every other position."""
    rng = np.random.default_rng(10)
    H, W = (W3, H3) if variant == "swapped" else (H3, W3)
    yy, xx = np.mgrid[0:H3, 0:W3]
    per_image = [[] for _ in range(N3)]
    for a in range(40):
        mask = np.zeros((H3, W3), bool)
        y0, x0 = int(rng.integers(0, H3 - 3)), int(rng.integers(0, W3 - 3))
        h, w = (int(rng.integers(20, 60)), int(rng.integers(20, 90))) if variant == "busy" else (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
        mask[y0:y0 + h, x0:x0 + w] = a % 17 != 5
        if variant == "busy":
            mask &= (yy + xx) % 2 == 0
        if variant == "swapped":
            mask = mask.T
        per_image[int(rng.integers(0, N3))].append((RR.mask_counts(mask), int(rng.integers(1, 40))))
    return TR._annotation_arrays(per_image), N3, H, W


class RleDecode(Entry):
    """camo_rle_decode of forty annotations on the free shape against rle_ref.decode bytewise.  BYTEWISE: camo_rle.h promises that two
    calls give the same bytes and test_decode_of_many_annotations_over_three_images compares the raw call's bytes with the wrapper's."""

    def build(self, variant):
        return BUILDERS["camo_rle_decode"](*_annotations(variant))

    def check(self, got):
        arrays, N, H, W = _annotations("case")
        want = RR.decode(*arrays, N, H, W)
        assert (want[1] == H * W).all() and want[0].any()
        _same_bytes(got, dict(zip(("labels", "ann_sum"), want)), "forty annotations")


# ---- guided filter and the segmentation measures -------------------------------------------------------------------------------------

class Guided(Entry):
    """camo_guided_filter on the free shape with the radius, eps and input kinds of one of test_guided's FILTER_CASES, q and coef against
    guided_ref within q_bound and coef_bounds (magnitudes from the reference).  BYTEWISE: test_filter_against_the_reference asserts two
    calls give the same bytes."""

    def __init__(self, i, shape=(N3, H3, W3)):
        (_, self.r, self.C, self.eps, self.gk, self.pk, _), self.i, self.shape = TGD.FILTER_CASES[i], i, shape

    @functools.lru_cache(maxsize=None)
    def _arrays(self, variant):
        seed = 1000 * self.i + (500 if variant == "busy" else 0)
        gk, pk = ("binary", "binary") if variant == "busy" else (self.gk, self.pk)
        N, H, W = self.shape
        guide = np.stack([GR.make_guide(gk, H, W, self.C, seed + n) for n in range(N)])
        p = np.stack([GR.make_p(pk, H, W, seed + n) for n in range(N)])
        return (_t(guide), _t(p)) if variant == "swapped" else (guide, p)

    def build(self, variant):
        return BUILDERS["camo_guided_filter"](*self._arrays(variant), self.C, self.r, self.eps)

    @functools.lru_cache(maxsize=None)
    def _refs(self):
        guide, p = self._arrays("case")
        return [GR.guided_filter(guide[n], p[n], self.r, self.eps) for n in range(len(p))]

    def check(self, got):
        for n, ref in enumerate(self._refs()):
            TGD._within(f"q, C = {self.C}, image {n}", got["q"][n], ref["q"], GR.q_bound(ref))
            TGD._within(f"coef, C = {self.C}, image {n}", got["coef"][n], ref["coef"], GR.coef_bounds(ref))


def _measure_maps(variant):
    """(maps fp32 [N, 3, H, W] with the prediction in channel 1, read in place as the modules' tests pass it; gt uint8 [N, H, W]) of
    test_seg_measures' first batch at 33 x 70; busy: uniform predictions over five blobs in every image."""
    pred, gt, _, _ = TS._images()[0]
    if variant == "busy":
        pred = np.stack([TS._uniform(33, 70, 40 + i) for i in range(3)])
        gt = np.stack([TS._blobs(33, 70, 50 + i, k=5) for i in range(3)])
    if variant == "swapped":
        pred, gt = _t(pred), _t(gt)
    maps = np.random.RandomState(11).uniform(0, 1, (pred.shape[0], 3) + pred.shape[1:]).astype(np.float32)
    maps[:, 1] = pred
    return maps, np.ascontiguousarray(gt)


class SegHistograms(Entry):
    """camo_seg_histograms on test_seg_measures' first batch against seg_measures_ref.table exactly; ``hist`` (accumulated into, and home of
    the centroid's 64-bit sums between the launches) and ``split`` (split[2 i] is the last-block ticket of the centroid kernel) are the
    dirty arrays.  BYTEWISE: _check_tables asserts two calls give the same bytes."""

    def build(self, variant):
        maps, gt = _measure_maps(variant)
        return BUILDERS["camo_seg_histograms"](maps, 1, gt)

    def check(self, got):
        _, _, hist, split = TS._images()[0]
        _same_bytes(got, {"hist": hist, "split": split}, "histograms")


class SegWeightedF(Entry):
    """camo_seg_weighted_f on test_seg_measures' first batch: n_fg exact, A_fg and A_bg within H W units of 2^-32 of the restatement, as
    test_seg_weighted_f._check.  BYTEWISE: that check asserts two calls give the same bytes (integer atomics after block-level sums)."""

    def build(self, variant):
        maps, gt = _measure_maps(variant)
        return BUILDERS["camo_seg_weighted_f"](maps, 1, gt)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _want():
        pred, gt, _, _ = TS._images()[0]
        return [SR.weighted_f_sums(pred[i], gt[i]) for i in range(len(pred))]

    def check(self, got):
        rows = got["sums"].tolist()
        for i, want in enumerate(self._want()):
            assert rows[i][0] == want[0]
            assert abs(rows[i][1] - want[1]) <= 33 * 70 and abs(rows[i][2] - want[2]) <= 33 * 70, (rows[i], want)


class SegCounts(Entry):
    """camo_seg_counts on the free shape with the inputs of test_counts_are_exact (values at the threshold, 0 and 1; gt bytes on both sides
    of 127) against rg_detect_ref.counts exactly.  BYTEWISE: that test asserts two calls give the same bytes."""

    @functools.lru_cache(maxsize=None)
    def _arrays(self, variant):
        rs = np.random.RandomState(12 + (variant == "busy"))
        maps = rs.uniform(0, 1, (N3, 3, H3, W3)).astype(np.float32)
        sel = rs.uniform(size=(N3, H3, W3))
        maps[:, 1][sel < 0.1] = 0.5
        maps[:, 1][(sel >= 0.1) & (sel < 0.15)] = 0.0
        maps[:, 1][(sel >= 0.15) & (sel < 0.2)] = 1.0
        gt = rs.choice(np.array([0, 127, 128, 255], np.uint8), (N3, H3, W3))
        if variant == "swapped":
            maps, gt = np.ascontiguousarray(maps.transpose(0, 1, 3, 2)), _t(gt)
        return maps, gt

    def build(self, variant):
        maps, gt = self._arrays(variant)
        return BUILDERS["camo_seg_counts"](maps, 1, gt, 0.5)

    def check(self, got):
        maps, gt = self._arrays("case")
        want = DR.counts(maps[:, 1], gt, 0.5)
        assert (want[:, :4].sum(1) == H3 * W3).all()
        _same_bytes(got, {"counts": want}, "counts")


ENTRIES = {
    "camo_canny": Canny(), "camo_canny_hysteresis": Hysteresis(), "camo_slic": Slic(), "camo_slic_connect": SlicConnect(), "camo_slic_update": SlicUpdate(),
    "camo_rg_region_graph": RegionGraph(), "camo_rg_region_graph_batch": RegionGraphBatch(), "camo_rg_node_targets": NodeTargets(),
    **{f"camo_instances-{c}-{'fill' if f else 'nofill'}": Instances(c, f) for c in (4, 8) for f in (False, True)},
    "camo_inst_match": InstMatch(), "camo_rle_runs": RleRuns(), "camo_rle_decode": RleDecode(),
    "camo_guided_filter-C1": Guided(6), "camo_guided_filter-C3": Guided(7),
    "camo_seg_histograms": SegHistograms(), "camo_seg_weighted_f": SegWeightedF(), "camo_seg_counts": SegCounts(),
}


@functools.lru_cache(maxsize=None)
def _clean(name):
    return ENTRIES[name].run("clean")


def test_the_table_names_every_pipeline_call_and_the_filter_cases_are_the_ones_meant():
    assert TGD.FILTER_CASES[6][1:4] == (3, 1, 1e-4) and TGD.FILTER_CASES[7][1:4] == (8, 3, 1e-6)
    assert {n.split("-")[0] for n in ENTRIES} == {
        "camo_canny", "camo_canny_hysteresis", "camo_slic", "camo_slic_connect", "camo_slic_update", "camo_rg_region_graph",
        "camo_rg_region_graph_batch", "camo_rg_node_targets", "camo_instances", "camo_inst_match", "camo_rle_runs", "camo_rle_decode",
        "camo_guided_filter", "camo_seg_histograms", "camo_seg_weighted_f", "camo_seg_counts"}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_point_on_caller_memory(name, variant):
    """One entry point, one variant (the module's docstring): guards intact after every call, the outputs held to the reference as the
    module's own test holds them, and -- under the BYTEWISE rule -- the declared outputs of the dirty variants byte-equal to clean's."""
    entry = ENTRIES[name]
    got = _clean(name) if variant == "clean" else entry.run(variant)
    entry.check(got)
    if variant != "clean" and entry.bytewise:
        _same_bytes(entry.declared(got), entry.declared(_clean(name)), f"{name}, {variant} against clean")


# ---- a carve one element short --------------------------------------------------------------------------------------------------
# The carves (*_carve in the .hip files) hand out 256-byte aligned pieces, so a piece taken one element short moves no address unless
# the piece ends within one element of a 256-byte boundary -- at 70 x 133 none does, and such a mistake would change nothing there.
# At 4865 = 19 * 256 + 1 pixels every piece of npix elements, whatever the element size, ends exactly one element past a boundary: a take of
# npix - 1 elements makes that piece, and the whole workspace, 256 bytes shorter.  The pieces behind it then begin inside it and the
# last one ends past the size *_workspace_bytes states, which is the size of the guarded buffer here.

CARVE_SHAPE = (1, 35, 139)
CARVED = {"camo_canny_hysteresis": Hysteresis(CARVE_SHAPE), "camo_slic_connect": SlicConnect(CARVE_SHAPE), "camo_instances": Instances(8, True, CARVE_SHAPE),
          "camo_guided_filter": Guided(6, CARVE_SHAPE)}


def test_the_carve_shape_ends_every_piece_one_element_past_a_boundary():
    n = CARVE_SHAPE[0] * CARVE_SHAPE[1] * CARVE_SHAPE[2]
    assert all(n * size % 256 == size for size in (1, 4, 8)) and CARVE_SHAPE[1] > 32 and CARVE_SHAPE[2] > 128


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CARVED))
def test_workspace_pieces_that_end_one_element_past_a_256_byte_boundary(name):
    """The entry points with per-pixel workspace pieces at 35 x 139 (the note above), workspace and outputs 0xFF, held to the reference
    as in the table above; the workspace guard is the check on the carve."""
    entry = CARVED[name]
    entry.check(execute(entry.build("case"), 0xFF))


# ---- the clears past their grid caps, on 0xFF memory ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_decode_clears_label_maps_of_more_than_2_to_20_pixels():
    """camo_rle_decode, N = 2 at 725 x 725: 1 051 250 pixels, past the 4096 blocks x 256 threads of one pass of rle_prefix_kernel's
    clear (its stride is (gridDim.x - A) * NT).  Two rectangle annotations, the buffers 0xFF: every pixel outside them must be 0.
    The second pass is the last 2674 pixels, rows 721 to 724 of image 1; the rectangles stay clear of them, so nothing paints
    over what the clear leaves."""
    N, H, W = 2, 725, 725
    assert N * H * W > 1 << 20
    a, b = np.zeros((H, W), bool), np.zeros((H, W), bool)
    a[100:300, 50:700] = True
    b[400:650, 10:715] = True
    arrays = TR._annotation_arrays([[(RR.mask_counts(a), 3)], [(RR.mask_counts(b), 7)]])
    got = execute(BUILDERS["camo_rle_decode"](arrays, N, H, W), 0xFF)
    want = RR.decode(*arrays, N, H, W)
    _same_bytes(got, dict(zip(("labels", "ann_sum"), want)), "725 x 725")
    assert got["labels"].sum() == 3 * a.sum() + 7 * b.sum() and not got["labels"][0][~a].any() and not got["labels"][1][~b].any()


@pytest.mark.gpu
@pytest.mark.parametrize("N,ids", [(2, 1023), (5, 511)])
def test_match_clears_overlap_tables_of_more_than_2_to_20_cells(N, ids):
    """camo_inst_match with N (P + 1) (G + 1) = 2^21 and 1.3 * 2^20 cells, past the 4096 blocks x 256 threads of one pass of
    im_clear_kernel: 64 x 64 maps of 4 x 4 blocks of random ids, one threshold, the buffers 0xFF, against inst_match_ref bytewise."""
    assert N * (ids + 1) ** 2 > 1 << 20
    pred = np.stack([IMR.blocks(64, 64, ids, 60 + n) for n in range(N)]).astype(np.int32)
    gt = np.stack([np.roll(IMR.blocks(64, 64, ids, 80 + n), 2, 1) for n in range(N)]).astype(np.int32)
    thr = (F(1, 2),)
    got = execute(BUILDERS["camo_inst_match"](pred, gt, ids, ids, None, thr), 0xFF)
    _same_bytes(got, IMR.match_batch(pred, gt, ids, ids, None, thr), f"{N} x {ids} ids")
    assert got["inter"].sum() == N * 64 * 64


@pytest.mark.gpu
def test_node_targets_clear_counts_of_more_than_2_to_19_ints():
    """camo_rg_node_targets with n_nodes = 131 109: 524 436 ints of ``counts``, past the 2048 blocks x 256 threads of one pass of
    rgtg_clear_kernel.  One 33 x 70 image whose region map sends 41 labels to nodes spread over the whole range, the last node and the
    first ones of the second pass among them; the buffers 0xFF.  Every other node must come out as -1, -1, -1.0f with counts 0."""
    n_nodes, lb = 131109, 41
    assert 4 * n_nodes > 1 << 19
    seg = RO.voronoi_segments(33, 70, lb - 1, 13).astype(np.int32)[None]
    seg[0, :2, :5] = 0
    rmap = (np.arange(lb, dtype=np.int64) * 3277 % n_nodes).astype(np.int32)[None]
    rmap[0, 1:5] = n_nodes - 1, 1 << 17, (1 << 17) + 1, (1 << 17) - 1
    assert len(np.unique(rmap)) == lb
    rs = np.random.RandomState(14)
    gt, inst, edge = TT._blobs(rs, 1, 33, 70), TT._blobs(rs, 1, 33, 70), TT._blobs(rs, 1, 33, 70, k=6)
    got = execute(BUILDERS["camo_rg_node_targets"](seg, rmap, [0, n_nodes], gt, inst, edge, n_nodes, 0, 1), 0xFF)
    want = TG.node_targets(seg, rmap, [0, n_nodes], gt, inst, edge, 0, 1, n_nodes)
    _same_bytes(got, dict(zip(("mask_t", "inst_t", "edge_t", "counts"), want)), "131 109 nodes")
    used = np.zeros(n_nodes, bool)
    used[rmap[0]] = True
    assert want[3][:, 0].sum() == 33 * 70 and (want[3][used, 0] > 0).all()
    assert not got["counts"][~used].any() and (got["mask_t"][~used] == -1).all() and (got["inst_t"][~used] == -1).all() and (got["edge_t"][~used] == -1.0).all()


@pytest.mark.gpu
def test_region_graph_clears_past_its_grid_on_a_dirty_workspace():
    """camo_rg_region_graph on rg_maps' perm64 (4096 labels): 73 728 accumulator doubles and 2^22 adjacency words, both past the
    256 blocks x 256 threads = 2^16 of one pass of rgf_clear_kernel -- the largest case of test_rg_graph_shapes passes the cap, so it
    is run once more with the workspace and the outputs 0xFF, against the oracle with that file's bounds."""
    assert 4096 * 18 > 1 << 16
    img, seg, canny = M.case("perm64")
    want = M.oracle("perm64")
    got = execute(BUILDERS["camo_rg_region_graph"](img, seg, canny.astype(np.uint8), 4096, want[1].shape[1]), 0xFF)
    _check_single_graph(got, want, TGS._std_bound("perm64", want))


@pytest.mark.gpu
def test_batched_region_graph_clears_past_its_grid_on_a_dirty_workspace():
    """camo_rg_region_graph_batch with nwords = N label_bound ceil(label_bound / 32) past the 2048 blocks x 256 threads = 2^19 of one
    pass of rgb_clear_kernel.  No case of test_rg_graph_shapes passes it: the largest, perm64 at N = 1 and label_bound 4096, has
    4096 * 128 = 2^19 words exactly (and 86 016 accumulators), one full pass.  N = 2 is therefore the smallest batch that can; its
    smallest bound, 2881 (2 * 2881 * 91 = 2^19 + 54), would leave the second pass 54 words of a label no map uses, so the case is
    N = 2 at label_bound 4096, perm64 twice: the second pass is then the whole adjacency of image 1, which must equal image 0's graph.
    Workspace and outputs 0xFF, against the oracle with the project's bounds; flat one-pixel regions have variance exactly 0."""
    lb = 4096
    assert 2 * lb * ((lb + 31) // 32) > 1 << 19 >= lb * ((lb + 31) // 32)
    img, seg, canny = (np.stack([a, a]) for a in M.case("perm64"))
    want = [M.oracle("perm64")] * 2
    got = execute(BUILDERS["camo_rg_region_graph_batch"](img, seg, canny.astype(np.uint8), lb, 2 * want[0][1].shape[1]), 0xFF)
    _check_batch_graph(got, want, "perm64 twice")
    d = _declared_batch_graph(got)
    assert (d["x"][:, TGS.STD_COLS + [14]] == 0).all()
    assert d["x"][:lb].tobytes() == d["x"][lb:].tobytes() and d["edge_attr"][:len(d["edge_attr"]) // 2].tobytes() == d["edge_attr"][len(d["edge_attr"]) // 2:].tobytes()
