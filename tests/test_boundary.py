"""Boundary IoU (include/camo_boundary.h): the numpy restatement tests/boundary_ref.py against scipy's erosion and hand
cases (CPU, no kernel), and the kernels against the restatement byte for byte (GPU).

Every raw GPU call places every buffer -- inputs, outputs, workspace -- between guard bytes (tests/guarded.py) and runs twice, on
memory filled with 0x00 and with 0xFF."""
import ctypes
import functools
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import boundary_ref as B
import inst_match_ref as R
import test_inst_match as M
from conftest import ROOT
from inst_match_ref import blocks as _blocks, score_table as _table
from raw_calls import BOUNDARY_MATCH_NAMES as MATCH_NAMES, BUILDERS, execute, same_bytes

from camouflage_multimodal_amd._lib import BD_STRIP as STRIP      # the column pass's strip height; test_header_constants holds it to the kernel's constant


def _discs(N, H, W, seed, ids=5):
    """[N, H, W] maps of overlapping discs with ids 1 .. ids on background 0 (a later disc covers an earlier one)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((N, H, W), np.int32)
    for n in range(N):
        for k in range(1, ids + 1):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, max(3, min(max(H, W), 40) // 2))
            out[n][(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = k
    return out


def _hand():
    pred, gt = np.zeros((1, 64, 64), np.int32), np.zeros((1, 64, 64), np.int32)
    pred[0, 10:50, 10:50], gt[0, 12:52, 12:52] = 1, 1
    return pred, gt


def _strips():
    """Thin strips (width 2d: boundary = mask) beside squares, d = 2.  Prediction 1 is a square shifted by a row against ground truth 1
    plus most of the strip that is ground truth 2; prediction 2 is the rest of the strip; prediction 3 is the outer ring of ground
    truth 3.  Under mask IoU 1 takes 1 and 2 takes 2; under the combined IoU 1 takes 2 and 2 goes empty."""
    g, p = np.zeros((1, 40, 128), np.int32), np.zeros((1, 40, 128), np.int32)
    g[0, 4:20, 4:20], g[0, 30:34, 4:104], g[0, 4:20, 40:60] = 1, 2, 3
    p[0, 5:21, 4:20], p[0, 30:34, 4:74], p[0, 30:34, 74:104], p[0, 4:20, 40:60] = 1, 1, 2, 3
    p[0, 6:18, 42:58] = 0
    return p, g


# ---- the label cases: name -> (labels [N, H, W] int32, d) ------------------------------------------------------------------

SIZES = ((1, 1), (1, 70), (70, 1), (33, 33), (45, 70), (130, 67))
LABEL_CASES = [f"discs_{H}x{W}_d{d}" for H, W in SIZES for d in (1, 2, 7, 40)] + [
    "all_one_d2", "all_one_d7", "squares_d1", "squares_d2", "squares_d7", "side_by_side", "row_wrap", "seams", "runs_d1", "runs_d7",
    "column_d2", "column_d40", "column_seam", "odd_labels", "discs_batch"]


def _squares(d):
    """45 x 70: a square of side 2d + 1 in the image's corner (1: its window just fits, one interior pixel), of side 2d in the opposite
    corner (2: none), of side 2d + 1 in the open (3: exactly one interior pixel) and of side 2d in the open (4: none)."""
    m = np.zeros((1, 45, 70), np.int32)
    a, b = 2 * d + 1, 2 * d
    m[0, :a, :a], m[0, 45 - b:, 70 - b:], m[0, 16:16 + a, 20:20 + a], m[0, 16:16 + b, 45:45 + b] = 1, 2, 3, 4
    return m


def _runs(d):
    """Runs of length 63, 64, 65 and 129 starting at x = 0, 1 and 63, each on 2d + 2 rows (so that its middle rows can be interior)
    with a label of its own."""
    rep, W = 2 * d + 2, 200
    m = np.zeros((1, 12 * rep, W), np.int32)
    k = 0
    for length in (63, 64, 65, 129):
        for start in (0, 1, 63):
            m[0, k * rep:(k + 1) * rep, start:start + length] = k + 1
            k += 1
    return m


@functools.lru_cache(maxsize=None)
def _label_case(name):
    m = re.fullmatch(r"discs_(\d+)x(\d+)_d(\d+)", name)
    if m:
        H, W, d = (int(v) for v in m.groups())
        return _discs(1, H, W, 100 + H + W), d
    if name.startswith("all_one"):
        return np.ones((1, 45, 70), np.int32), int(name.split("_d")[1])
    if name.startswith("squares"):
        d = int(name.split("_d")[1])
        return _squares(d), d
    if name == "side_by_side":
        lab = np.ones((1, 20, 40), np.int32)
        lab[0, :, 20:] = 2
        return lab, 2
    if name == "row_wrap":                            # the label ends every row and begins the next: joined, the runs of 4 would be 8 long
        lab = np.zeros((1, 12, 70), np.int32)         # and columns 2 .. 3 and 66 .. 67 interior
        lab[0, :, 66:], lab[0, :, :4] = 1, 1
        return lab, 2
    if name == "seams":                               # the same label on both sides of every image seam
        return np.full((3, 9, 70), 4, np.int32), 2
    if name.startswith("runs"):
        d = int(name.split("_d")[1])
        return _runs(d), d
    if name in ("column_d2", "column_d40"):           # a column run over more than two strips of the column pass
        d = int(name.split("_d")[1])
        lab = np.zeros((1, 2 * STRIP + 10, 90), np.int32)
        lab[0, 3:2 * STRIP + 6, 2:88] = 1
        return lab, d
    if name == "column_seam":                         # the label changes exactly where one strip ends and the next begins
        lab = np.ones((1, 2 * STRIP + 10, 20), np.int32)
        lab[0, STRIP:] = 2
        return lab, 2
    if name == "odd_labels":
        lab = np.zeros((1, 33, 33), np.int32)
        lab[0, 2:14, 2:14], lab[0, 16:30, 4:16], lab[0, 16:30, 16:28], lab[0, 0, 20:] = 1 << 30, 3, -1, -1
        return lab, 2
    if name == "discs_batch":
        return _discs(3, 45, 70, 7), 2
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _label_ref(name):
    lab, d = _label_case(name)
    return B.boundary_labels_ref(lab, d)


# ---- the match cases: name -> (pred, gt [N, H, W], d, P, G, table, thresholds) ----------------------------------------------

MATCH_CASES = ["hand", "d_past_side", "strips", "ties", "one_id", "ids_300", "one_threshold", "sixteen_thresholds", "out_of_range", "batch"]


@functools.lru_cache(maxsize=None)
def _match_case(name):
    table, thr, d = None, R.COCO, 2
    if name == "hand":
        (pred, gt), P, G = _hand(), 2, 2
    elif name == "d_past_side":
        pred, gt, P, G, table, d = _blocks(32, 32, 8, 13)[None], np.roll(_blocks(32, 32, 8, 13), 1, 0)[None], 8, 8, _table(1, 8, 3), 40
    elif name == "strips":
        (pred, gt), P, G, thr = _strips(), 3, 3, (F(1, 4), F(2, 5), F(1, 2))
    elif name == "ties":                              # one row: every pixel is boundary, both fractions are 1/2 with either ground truth
        pred, gt, P, G, thr, d = np.array([[[1, 1, 1, 1]]]), np.array([[[1, 1, 2, 2]]]), 1, 2, (F(10, 20), F(11, 20)), 1
    elif name == "one_id":
        pred, gt, P, G = (_discs(1, 40, 40, 21, 2) > 0).astype(np.int64), (_discs(1, 40, 40, 22, 2) > 0).astype(np.int64), 1, 1
        thr = (F(1, 10), F(1, 2))
    elif name == "ids_300":
        idx = np.arange(1600).reshape(40, 40)
        pred, gt, P, G, table, thr, d = ((idx // 5) % 300 + 1)[None], (((idx + 1) // 5) % 300 + 1)[None], 300, 300, _table(1, 300, 6), (F(1, 2), F(13, 20), F(3, 4)), 1
    elif name == "one_threshold":
        pred, gt, P, G, thr = _discs(1, 48, 56, 31), np.roll(_discs(1, 48, 56, 31), 1, 2), 5, 5, (F(3, 10),)
    elif name == "sixteen_thresholds":
        pred, gt, P, G, table = _discs(1, 48, 56, 32), np.roll(_discs(1, 48, 56, 32), 1, 1), 5, 5, _table(1, 5, 18)
        thr = tuple(F(n, 32) for n in range(2, 33, 2))
    elif name == "out_of_range":
        pred, gt, P, G = _blocks(24, 40, 5, 12, 8)[None].copy(), np.roll(_blocks(24, 40, 5, 12, 8), 2, 0)[None].copy(), 5, 5
        pred[0, 0, :7], pred[0, 3:9, 4:12], gt[0, 5, :11], gt[0, 0, 2:5] = -1, P + 1, G + 7, -1
        thr = (F(1, 4), F(1, 2))
    elif name == "batch":
        pred = np.stack([_discs(1, 37, 29, 40 + n)[0] for n in range(5)])
        gt = np.stack([np.roll(pred[n], (n % 3, n % 2), (0, 1)) for n in range(5)])
        P, G, table, thr = 5, 5, _table(5, 5, 19), (F(1, 4), F(1, 2), F(3, 4))
    else:
        raise KeyError(name)
    return pred.astype(np.int32), gt.astype(np.int32), d, P, G, table, thr


@functools.lru_cache(maxsize=None)
def _match_maps(name):
    pred, gt, d = _match_case(name)[:3]
    return B.boundary_labels_ref(pred, d), B.boundary_labels_ref(gt, d)


@functools.lru_cache(maxsize=None)
def _match_ref(name):
    pred, gt, d, P, G, table, thr = _match_case(name)
    return B.boundary_match_ref(pred, gt, *_match_maps(name), P, G, table, thr)


def _same(got, want, what, names=MATCH_NAMES):
    assert all(np.asarray(want[k]).dtype == np.int32 for k in names)
    same_bytes(got, want, what, names)


# ---- CPU: the restatement itself, and the host side of the binding ----------------------------------------------------------

def test_restated_boundary_is_scipys_erosion_of_the_padded_mask():
    ndimage = pytest.importorskip("scipy.ndimage")
    for trial in range(12):
        lab = _discs(1, 24 + trial, 40 - trial, trial)[0]
        if trial == 3:
            lab[:] = 2                                # an all-one-label image
        for d in (1, 2, 3, 4):
            got = B.boundary_labels_ref(lab, d)
            for k in np.unique(lab[lab > 0]):
                m = lab == k
                eroded = ndimage.binary_erosion(np.pad(m, 1), np.ones((3, 3)), iterations=d, border_value=1)[1:-1, 1:-1]
                assert ((got == k) == (m & ~eroded)).all(), (trial, d, k)
                assert (got == k).sum() >= 1          # every instance with a pixel keeps a boundary pixel
            assert (got[lab <= 0] == 0).all()


def test_every_instance_keeps_a_boundary_pixel_and_labels_below_one_give_nothing():
    lab = _discs(2, 30, 41, 50, 6)
    lab[0, :3], lab[1, 5:9, 5:9] = -1, 1 << 30
    for d in (1, 3, 50):
        got = B.boundary_labels_ref(lab, d)
        for n in range(2):
            for k in np.unique(lab[n][lab[n] > 0]):
                assert (got[n] == k).sum() >= 1 and ((got[n] == k) <= (lab[n] == k)).all()
        assert (got[lab <= 0] == 0).all()
    assert (B.boundary_labels_ref(lab, 50) == np.maximum(lab, 0)).all()


def test_boundary_distance_is_round_half_up_of_the_diagonal():
    from camouflage_multimodal_amd.boundary import boundary_distance
    assert [boundary_distance(*s) for s in ((256, 256), (480, 640), (768, 1024), (1, 1))] == [7, 16, 26, 1]
    for H in range(1, 65):
        for W in range(1, 65):
            assert boundary_distance(H, W) == max(1, int(round(0.02 * math.hypot(H, W)))), (H, W)
    assert boundary_distance(300, 400, F(1, 10)) == 50 and boundary_distance(300, 400, 0.5) == 250 and boundary_distance(3, 4, 1) == 5
    for bad in (dict(H=0, W=4), dict(H=4, W=-1), dict(H=2.5, W=4), dict(H=True, W=4)):
        with pytest.raises(ValueError, match="must be a positive integer"):
            boundary_distance(**bad)
    for ratio in (0, -1, 2, "1/50", None, float("nan"), True):
        with pytest.raises(ValueError, match="ratio"):
            boundary_distance(10, 10, ratio)


def test_hand_case_matches_under_mask_iou_and_not_under_the_combined_one():
    pred, gt = _hand()
    pb, gb = B.boundary_labels_ref(pred, 2), B.boundary_labels_ref(gt, 2)
    out = B.boundary_match_ref(pred, gt, pb, gb, 1, 1)
    assert out["inter"][0, 1, 1] == 1444 and 1600 + 1600 - 1444 == 1756
    assert out["pred_rows"][0].tolist() == [[1600, 0, 1, 1444, 304, 8]] and out["gt_area"][0].tolist() == [[1600, 304]]
    assert out["inter_bd"][0, 1, 1] == 8 and 304 + 304 - 8 == 600
    assert not out["match"].any() and not out["gt_match"].any()                  # 8 / 600 is below every COCO threshold
    plain = R.match_batch(pred, gt, 1, 1)
    assert plain["match"][0, :, 0].tolist() == [1] * 7 + [0] * 3                 # 1444 / 1756 = 0.82: matched from 0.50 to 0.80
    assert B.combined(1444, 1756, 8, 600) == (8, 600) and B.combined(1, 2, 3, 6) == (1, 2) and B.combined(5, 9, 0, 0) == (0, 1)


def test_a_distance_past_the_sides_gives_the_mask_match():
    pred, gt, d, P, G, table, thr = _match_case("d_past_side")
    pb, gb = _match_maps("d_past_side")
    assert (pb == np.maximum(pred, 0)).all() and (gb == np.maximum(gt, 0)).all()
    out, plain = _match_ref("d_past_side"), R.match_batch(pred, gt, P, G, table, thr)
    assert plain["match"].any()
    _same(out, plain, "d past side", ("inter", "match", "gt_match", "counts"))
    assert (out["pred_rows"][..., :4] == plain["pred_rows"]).all() and (out["gt_area"][..., 0] == plain["gt_area"]).all()
    assert (out["inter_bd"] == out["inter"]).all()


def test_the_strips_case_orders_differently_under_each_of_the_three_ious():
    pred, gt, d, P, G, table, thr = _match_case("strips")
    pb, gb = _match_maps("strips")
    both, mask, bd = _match_ref("strips")["match"][0], R.match_batch(pred, gt, P, G, None, thr)["match"][0], R.match_batch(pb, gb, P, G, None, thr)["match"][0]
    assert mask[0].tolist() == [1, 2, 3] and both[0].tolist() == [2, 0, 3]      # prediction 1 takes the strip, prediction 2 goes empty
    assert (both != mask).any() and (both != bd).any() and bd[2].tolist() == [2, 0, 3] and both[2].tolist() == [0, 0, 0]
    ties = _match_ref("ties")
    assert ties["match"][0].tolist() == [[1], [0]] and ties["pred_rows"][0].tolist() == [[4, 0, 1, 2, 4, 2]]      # equal fractions: the smaller id


def _is_the_mask_match(got, plain, what):
    """`got`, the combined match with the label maps as their own boundary maps, against `plain`, the mask-only match: bd_cand keeps the
    mask fraction where the two are equal, so every shared output is the same bytes and the boundary fields repeat the mask's."""
    names = ("inter", "match", "gt_match", "counts", "pred_rows", "gt_area")
    _same({**got, "pred_rows": np.ascontiguousarray(got["pred_rows"][..., :4]), "gt_area": np.ascontiguousarray(got["gt_area"][..., 0])}, plain, what, names)
    assert got["inter_bd"].tobytes() == got["inter"].tobytes(), what
    assert (got["pred_rows"][..., 4] == got["pred_rows"][..., 0]).all() and (got["pred_rows"][..., 5] == got["pred_rows"][..., 3]).all(), what
    assert (got["gt_area"][..., 1] == got["gt_area"][..., 0]).all(), what


def test_with_the_label_maps_as_boundary_maps_the_restated_match_is_the_mask_match():
    for name in M.CASES:
        pred, gt, P, G, table, thr = M._case(name)
        _is_the_mask_match(B.boundary_match_ref(pred, gt, pred, gt, P, G, table, thr), M._ref(name), name)


def test_argument_errors_by_name_and_no_cpu_path():
    from camouflage_multimodal_amd import boundary as bd
    from camouflage_multimodal_amd._lib import CamoError
    a = torch.zeros(2, 4, 4, dtype=torch.int32)
    for call in (bd.boundary_labels, lambda x, **kw: bd.match_instances_boundary(x, x, **kw)):
        for kw, word in (({"distance": 0}, "distance"), ({"distance": 4097}, "distance"), ({"distance": 2.0}, "distance"), ({"distance": True}, "distance"),
                         ({"ratio": 0}, "ratio"), ({"ratio": 1.5}, "ratio"), ({"ratio": "x"}, "ratio")):
            with pytest.raises(ValueError, match=word):
                call(a, **kw)
    with pytest.raises(ValueError, match="labels must be int32"):
        bd.boundary_labels(a.long())
    with pytest.raises(ValueError, match=r"need labels \[N, H, W\]"):
        bd.boundary_labels(a[None])
    with pytest.raises(ValueError, match="labels must be a tensor"):
        bd.boundary_labels(a.numpy())
    for kw, word in (({"max_pred": 0}, "max_pred"), ({"max_gt": 1025}, "max_gt"), ({"thresholds": ()}, "thresholds"), ({"thresholds": [1.5]}, "thresholds"),
                     ({"pred_table": torch.zeros(2, 3, 7, dtype=torch.int64)}, "pred_table"), ({"pred_boundary": a[:1]}, "pred_boundary"),
                     ({"gt_boundary": a.long()}, "gt_boundary"), ({"pred_boundary": a.numpy()}, "pred_boundary")):
        with pytest.raises(ValueError, match=word):
            bd.match_instances_boundary(a, a, **kw)
    with pytest.raises(ValueError, match="gt_labels of pred_labels' shape"):
        bd.match_instances_boundary(a, a[:1])
    with pytest.raises(ValueError, match="gt_labels must be int32"):
        bd.match_instances_boundary(a, a.float())
    m = torch.zeros(2, 4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="pred_masks must be a bool tensor"):
        bd.boundary_iou(a, m)
    with pytest.raises(ValueError, match="gt_masks of pred_masks' shape"):
        bd.boundary_iou(m, m[:1])
    with pytest.raises(ValueError, match="distance"):
        bd.boundary_iou(m, m, distance=0)
    with pytest.raises(CamoError, match="labels is on cpu"):                    # good arguments, CPU tensors: no fallback
        bd.boundary_labels(a)
    with pytest.raises(CamoError, match="pred_labels is on cpu"):
        bd.match_instances_boundary(a, a, distance=3, pred_boundary=a, gt_boundary=a)
    with pytest.raises(CamoError, match="pred_masks is on cpu"):
        bd.boundary_iou(m, m)
    opts = {"thresholds": R.COCO, "max_gt": 64}
    assert bd.boundary_options(None, opts) is None and bd.boundary_options(True, opts) == {"ratio": F(1, 50), "distance": None}
    assert bd.boundary_options({"distance": 5, "ratio": 0.1}, opts) == {"ratio": F(1, 10), "distance": 5}
    with pytest.raises(ValueError, match="boundary needs match"):
        bd.boundary_options(True, None)
    for bad, word in (({"d": 3}, "boundary must be"), (3, "boundary must be"), ({"distance": 0}, "distance"), ({"ratio": 7}, "ratio")):
        with pytest.raises(ValueError, match=word):
            bd.boundary_options(bad, opts)


def test_records_carry_instance_match_records_keys_and_the_boundary_figures():
    """boundary_match_records on the restatement's integers (CPU tensors: the copy is a no-op), and InstanceAP on them."""
    from camouflage_multimodal_amd import InstanceAP, instance_match_records
    from camouflage_multimodal_amd.boundary import boundary_match_records
    pred, gt = _hand()
    pb, gb = B.boundary_labels_ref(pred, 2), B.boundary_labels_ref(gt, 2)
    out = {k: torch.from_numpy(v) for k, v in B.boundary_match_ref(pred, gt, pb, gb, 1, 1).items()}
    out.update(thresholds=R.COCO, distance=2)
    rec, = boundary_match_records(out)
    plain = {k: torch.from_numpy(v) for k, v in R.match_batch(pred, gt, 1, 1).items()}
    plain["thresholds"] = R.COCO
    base, = instance_match_records(plain)
    assert set(base) <= set(rec) and set(base["predictions"][0]) <= set(rec["predictions"][0]) and rec["distance"] == 2
    p, = rec["predictions"]
    assert p["boundary_area"] == 304 and p["best_boundary_iou"] == 8 / 600 and p["best_mask_iou"] == 1444 / 1756 and p["best_iou"] == 8 / 600
    assert p["matches"] == [0] * 10 and p["best_gt"] == 1 and [t["tp"] for t in rec["per_threshold"]] == [0] * 10
    assert rec["pq"] is None and rec["n_pred"] == rec["n_gt"] == 1
    assert InstanceAP().add([rec], [[0.9]]).result()["AP"] == 0.0 and InstanceAP().add([base], [[0.9]]).result()["AP"] == pytest.approx(0.7)


def test_header_constants():
    from camouflage_multimodal_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "camo_boundary.h")).read(), flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    assert m["CAMO_BD_MAX_DISTANCE"] == "(1 << 12)" and _lib.BD_MAX_DISTANCE == 1 << 12
    assert int(m["CAMO_BD_STRIP"]) == _lib.BD_STRIP == STRIP
    kernel = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "boundary.h")).read()
    assert int(re.search(r"constexpr int BD_STRIP = (\d+);", kernel).group(1)) == STRIP      # the kernel's own constant
    assert int(m["CAMO_BD_ROW_FIELDS"]) == _lib.BD_ROW_FIELDS == 6 and int(m["CAMO_BD_GT_FIELDS"]) == _lib.BD_GT_FIELDS == 2
    assert "PARITY UNPINNED" in open(os.path.join(ROOT, "include", "camo_boundary.h")).read() and _lib.ABI_VERSION == 13
    assert _lib.symbols("camo_boundary.h") == ("camo_boundary_labels_workspace_bytes", "camo_boundary_labels", "camo_boundary_match_workspace_bytes",
                                               "camo_boundary_match")


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    ws = L.camo_boundary_labels_workspace_bytes
    assert ws(1, 1, 1, 1) == 256 and ws(2, 45, 70, 7) == 6400 and ws(1, 8, 8, 4096) > 0 and ws(16, 768, 1024, 26) == 16 * 768 * 1024
    for bad in ((0, 8, 8, 1), (65536, 1, 1, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8192, 8193, 1), (17, 8192, 8192, 1), (1, 8, 8, 0), (1, 8, 8, -2), (1, 8, 8, 4097)):
        assert ws(*bad) == 0, bad
    p, q, big = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), 1 << 40
    good = dict(labels=p, N=2, H=8, W=8, d=2, out=q, ws=ctypes.c_void_p(0x300000), nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return L.camo_boundary_labels(a["labels"], a["N"], a["H"], a["W"], a["d"], a["out"], a["ws"], a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=8192, W=8193), dict(d=0), dict(d=4097), dict(labels=None), dict(out=None), dict(ws=None),
               dict(out=p), dict(out=ctypes.c_void_p(0x100000 + 2 * 8 * 8 * 4 - 4)), dict(labels=ctypes.c_void_p(0x200000 + 4)),
               dict(ws=ctypes.c_void_p(0x300080)), dict(nbytes=ws(2, 8, 8, 2) - 1), dict(nbytes=0)):
        assert call(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()
    wm = L.camo_boundary_match_workspace_bytes
    assert wm(1, 1, 1, 1, 1, 1) > 0 and wm(1, 1, 1, 1, 1, 1) % 256 == 0 and wm(2, 8, 8, 64, 64, 10) > L.camo_inst_match_workspace_bytes(2, 8, 8, 64, 64, 10)
    for bad in ((0, 8, 8, 4, 4, 1), (1, 0, 8, 4, 4, 1), (1, 8, 8, 0, 4, 1), (1, 8, 8, 1025, 4, 1), (1, 8, 8, 4, 0, 1), (1, 8, 8, 4, 1025, 1), (1, 8, 8, 4, 4, 0),
                (1, 8, 8, 4, 4, 17), (64, 8, 8, 1024, 1024, 16)):
        assert wm(*bad) == 0, bad
    thr = (ctypes.c_int32 * 16)(*range(10, 26))
    goodm = dict(pl=p, gl=p, pb=p, gb=p, N=2, H=8, W=8, P=4, G=4, table=p, rows=4, thr=thr, den=25, T=10, inter=p, inter_bd=p, pred_rows=p, gt_area=p, match=p,
                 gt_match=p, counts=p, ws=p, nbytes=big)

    def callm(**kw):
        a = dict(goodm, **kw)
        return L.camo_boundary_match(a["pl"], a["gl"], a["pb"], a["gb"], a["N"], a["H"], a["W"], a["P"], a["G"], a["table"], a["rows"], a["thr"], a["den"],
                                     a["T"], a["inter"], a["inter_bd"], a["pred_rows"], a["gt_area"], a["match"], a["gt_match"], a["counts"], a["ws"],
                                     a["nbytes"], None)
    for kw in [dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(P=0), dict(P=1025), dict(G=0), dict(G=1025), dict(N=64, P=1024, G=1024), dict(T=0), dict(T=17),
               dict(den=0), dict(den=1001), dict(den=18), dict(thr=None), dict(thr=(ctypes.c_int32 * 16)(0, *range(11, 26))), dict(rows=0),
               dict(table=ctypes.c_void_p(0x100004)), dict(pl=None), dict(gl=None), dict(pb=None), dict(gb=None), dict(inter=None), dict(inter_bd=None),
               dict(pred_rows=None), dict(gt_area=None), dict(match=None), dict(gt_match=None), dict(counts=None), dict(ws=None),
               dict(ws=ctypes.c_void_p(0x100080)), dict(nbytes=wm(2, 8, 8, 4, 4, 10) - 1), dict(nbytes=0)]:
        assert callm(**kw) == -1, kw
        assert L.camo_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _raw_labels(lab, d, fill):
    """camo_boundary_labels with every buffer -- input, output, workspace -- between guard bytes filled with `fill` -> out as numpy."""
    return execute(BUILDERS["camo_boundary_labels"](lab, d), fill)["out"]


def _raw_match(pred, gt, pb, gb, P, G, table, thr, fill):
    return execute(BUILDERS["camo_boundary_match"](pred, gt, pb, gb, P, G, table, thr), fill)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LABEL_CASES)
def test_boundary_labels_equal_the_restatement_bytewise(name):
    lab, d = _label_case(name)
    want = _label_ref(name)
    for fill in (0x00, 0xFF):
        got = _raw_labels(lab, d, fill)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (name, fill, np.argwhere(got != want)[:5].tolist())


def test_the_label_cases_hold_what_their_names_say():
    for d in (1, 2, 7):
        want = _label_ref(f"squares_d{d}")[0]
        lab = _label_case(f"squares_d{d}")[0][0]
        interior = (lab > 0) & (want == 0)
        assert interior.sum() == 2 and interior[16 + d, 20 + d] and interior[d, d]      # the centres of the two squares of side 2d + 1, nothing else
    wrap = _label_ref("row_wrap")
    assert (wrap == _label_case("row_wrap")[0]).all()                # runs of 4: nothing is interior at d = 2
    col = _label_ref("column_d40")[0]
    assert ((col == 0) & (_label_case("column_d40")[0][0] == 1)).sum() == (2 * STRIP + 3 - 80) * (86 - 80)
    assert (_label_ref("runs_d7")[0] == 0)[7:9].sum() == 2 * (63 - 14 + 200 - 63) and (_label_ref("seams")[:, 0] == 4).all()
    odd, lab = _label_ref("odd_labels")[0], _label_case("odd_labels")[0][0]
    assert (odd[lab <= 0] == 0).all() and odd[2, 2] == 1 << 30 and odd[8, 8] == 0 and odd[20, 15] == 3 and odd[20, 10] == 0


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes_and_a_batch_gives_its_images():
    lab, d = _label_case("discs_batch")
    whole, again = _raw_labels(lab, d, 0x00), _raw_labels(lab, d, 0xFF)
    assert whole.tobytes() == again.tobytes()
    for n in range(len(lab)):
        assert _raw_labels(lab[n:n + 1], d, 0xFF).tobytes() == whole[n:n + 1].tobytes(), n
    pred, gt, d, P, G, table, thr = _match_case("batch")
    pb, gb = _match_maps("batch")
    both = _raw_match(pred, gt, pb, gb, P, G, table, thr, 0x00)
    _same(_raw_match(pred, gt, pb, gb, P, G, table, thr, 0xFF), both, "second call")
    for n in range(len(pred)):
        one = _raw_match(pred[n:n + 1], gt[n:n + 1], pb[n:n + 1], gb[n:n + 1], P, G, table[n:n + 1], thr, 0xFF)
        _same(one, {k: both[k][n:n + 1] for k in MATCH_NAMES}, f"image {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", MATCH_CASES)
def test_boundary_match_equals_the_restatement_bytewise(name):
    pred, gt, d, P, G, table, thr = _match_case(name)
    pb, gb = _match_maps(name)
    for fill in (0x00, 0xFF):
        _same(_raw_match(pred, gt, pb, gb, P, G, table, thr, fill), _match_ref(name), (name, fill))


@pytest.mark.gpu
@pytest.mark.parametrize("name", M.CASES)
def test_with_the_label_maps_as_boundary_maps_the_match_is_camo_inst_matchs_bytewise(name):
    """The two instantiations of the one match kernel, held to each other on test_inst_match's cases."""
    pred, gt, P, G, table, thr = M._case(name)
    plain = M._raw(pred, gt, P, G, table, thr)
    for fill in (0x00, 0xFF):
        _is_the_mask_match(_raw_match(pred, gt, pred, gt, P, G, table, thr, fill), plain, (name, fill))


@pytest.mark.gpu
def test_a_distance_past_the_sides_gives_camo_inst_matchs_own_outputs():
    from camouflage_multimodal_amd import match_instances
    from camouflage_multimodal_amd.boundary import boundary_labels, match_instances_boundary
    pred, gt, d, P, G, table, thr = _match_case("d_past_side")
    pl, gl, tab = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(table).cuda()
    assert torch.equal(boundary_labels(pl, d), pl.clamp(min=0))
    out, plain = match_instances_boundary(pl, gl, tab, None, G, thr, distance=d), match_instances(pl, gl, tab, None, G, thr)
    for k in ("inter", "match", "gt_match", "counts"):
        assert torch.equal(out[k], plain[k]), k
    assert torch.equal(out["pred_rows"][..., :4], plain["pred_rows"]) and torch.equal(out["gt_area"][..., 0], plain["gt_area"])
    assert torch.equal(out["inter_bd"], out["inter"]) and out["distance"] == d


@pytest.mark.gpu
def test_the_python_calls_are_the_raw_calls():
    from camouflage_multimodal_amd.boundary import boundary_iou, boundary_labels, boundary_match_records, match_instances_boundary
    for name in ("strips", "out_of_range", "batch"):
        pred, gt, d, P, G, table, thr = _match_case(name)
        pl, gl = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
        tab = None if table is None else torch.from_numpy(table).cuda()
        out = match_instances_boundary(pl, gl, tab, None if tab is not None else P, G, thr, distance=d)
        want = _match_ref(name)
        _same({k: out[k].cpu().numpy() for k in MATCH_NAMES}, want, name)
        assert (out["pred_boundary"].cpu().numpy() == _match_maps(name)[0]).all() and (out["gt_boundary"].cpu().numpy() == _match_maps(name)[1]).all()
        given = match_instances_boundary(pl, gl, tab, None if tab is not None else P, G, thr, pred_boundary=out["pred_boundary"], gt_boundary=out["gt_boundary"])
        _same({k: given[k].cpu().numpy() for k in MATCH_NAMES}, want, name + " (maps given)")
        assert given["distance"] is None
        for n, r in enumerate(boundary_match_records(out)):
            assert [t["tp"] for t in r["per_threshold"]] == (want["match"][n] > 0).sum(axis=1).tolist() and r["distance"] == d
            assert [p["boundary_area"] for p in r["predictions"]] == [int(want["pred_rows"][n, p["id"] - 1, 4]) for p in r["predictions"]]
    lab = torch.from_numpy(_label_case("discs_45x70_d2")[0]).cuda()
    assert (boundary_labels(lab[0], 2).cpu().numpy() == _label_ref("discs_45x70_d2")).all()            # [H, W] goes in as one image
    assert (boundary_labels(torch.from_numpy(_discs(1, 128, 128, 3)).cuda()).cpu().numpy() == B.boundary_labels_ref(_discs(1, 128, 128, 3), 4)).all()      # d = round(0.02 x 181)
    pred, gt = _hand()
    got, = boundary_iou(torch.from_numpy(pred > 0).cuda(), torch.from_numpy(gt > 0).cuda(), distance=2)
    assert got == {"boundary_iou": 8 / 600, "mask_iou": 1444 / 1756, "distance": 2}
    empty, = boundary_iou(torch.zeros(8, 8, dtype=torch.bool).cuda(), torch.zeros(8, 8, dtype=torch.bool).cuda())
    assert empty == {"boundary_iou": 0.0, "mask_iou": 0.0, "distance": 1}
