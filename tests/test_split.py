"""The instance splitter (include/camo_split.h): camo_split_instances against tests/split_ref.py, byte for byte.

CPU: the restatement's distance transform against scipy's where scipy is importable, its hand cases, every ValueError and CamoError of
camouflage_multimodal_amd/split.py, the library's argument checks with pointers that are never dereferenced, and -- for every input
of the GPU tests -- a test that shows from the restatement alone that the input has the property it is named for, so that no case
passes while it exercises nothing.  GPU: every buffer of every call sits between guards on memory the call did not clear
(tests/guarded.py, tests/raw_calls.py) and is compared byte for byte.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import split_ref as R
from conftest import ROOT
from instances_ref import components
from raw_calls import Call, execute, same_bytes

NAMES = ("labels", "table", "counts")
DEFAULT = dict(ratio=(7, 10), min_core=0, max_split=4, rows=64)


def _side_limit():
    text = open(os.path.join(ROOT, "include", "camo_seg_measures.h")).read()
    return int(re.search(r"#define\s+CAMO_SEG_WF_MAX_SIDE\s+(\d+)", text).group(1))


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def _disc(lab, cy, cx, r, value):
    yy, xx = np.mgrid[:lab.shape[0], :lab.shape[1]]
    lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value


def _dumbbell(lab, cy, cx0, cx1, r, value, half=1):
    """Two discs of radius r on one row, joined by a bar of 2 half + 1 rows."""
    _disc(lab, cy, cx0, r, value)
    _disc(lab, cy, cx1, r, value)
    lab[cy - half:cy + half + 1, cx0:cx1 + 1] = value


def _two_discs():
    lab = np.zeros((1, 40, 64), np.int32)
    _disc(lab[0], 20, 22, 12, 1)
    _disc(lab[0], 20, 42, 12, 1)
    return lab


def _noise(H, W, density, seed):
    mask = np.random.RandomState(seed).rand(H, W) < density
    lab, n = components(mask, 8)
    assert n <= R.MAX_ID
    return lab[None]


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (labels int32 [N, H, W], parameters of the call).  Read-only: the arrays are shared."""
    p = dict(DEFAULT)
    if name == "two_discs":
        lab = _two_discs()
    elif name == "two_discs_low_ratio":
        lab, p["ratio"] = _two_discs(), (3, 10)
    elif name == "bisector":                                  # centres 18 columns apart: column 29 is equidistant
        lab = np.zeros((1, 32, 60), np.int32)
        _disc(lab[0], 16, 20, 10, 1)
        _disc(lab[0], 16, 38, 10, 1)
    elif name == "own_id":                                    # a dumbbell with a long thin bar above a fat blob of another id
        lab = np.zeros((1, 48, 72), np.int32)
        _dumbbell(lab[0], 10, 10, 60, 7, 1)
        _disc(lab[0], 26, 35, 12, 2)
    elif name == "concave":                                   # a C: spine on the left, two arms, a fat end on the top arm and one on the spine
        lab = np.zeros((1, 40, 56), np.int32)
        lab[0, 4:36, 2:5] = 1
        lab[0, 4:7, 2:50] = 1
        lab[0, 33:36, 2:50] = 1
        _disc(lab[0], 10, 44, 6, 1)
        _disc(lab[0], 20, 8, 6, 1)
    elif name.startswith("core_drop"):                        # discs of radius 12 and 9: the smaller core's area decides
        lab = np.zeros((1, 40, 64), np.int32)
        _disc(lab[0], 20, 16, 12, 1)
        _disc(lab[0], 20, 36, 9, 1)
        small = min(R.split_image(lab[0])[3]["core_areas"])
        big = max(R.split_image(lab[0])[3]["core_areas"])
        p["min_core"] = {"at": small, "below": small - 1, "above": small + 1, "all": big + 1}[name.split("_")[-1]]
    elif name in ("slot_limit", "truncation"):                # three dumbbells, ids 1 .. 3
        lab = np.zeros((1, 48, 32), np.int32)
        for k in range(3):
            _dumbbell(lab[0], 8 + 16 * k, 9, 21, 6, k + 1, half=0)
        if name == "slot_limit":
            p["max_split"] = 2
        else:
            p["rows"] = 3
    elif name == "diagonal_ids":                              # one-pixel bars: every pixel is a core pixel; id 2's two bars touch id 1's ends diagonally
        lab = np.zeros((1, 8, 20), np.int32)
        lab[0, 2, 2:7] = 2
        lab[0, 3, 7:12] = 1
        lab[0, 4, 12:17] = 2
    elif name == "tile_corner":                               # id 1: the neck crosses (32, 32); id 2: a core lies on the corner (32, 96)
        lab = np.zeros((1, 64, 128), np.int32)
        _disc(lab[0], 22, 22, 9, 1)
        _disc(lab[0], 42, 42, 9, 1)
        for t in range(22, 43):
            lab[0, t - 1:t + 2, t - 1:t + 2] = 1
        _dumbbell(lab[0], 32, 72, 96, 9, 2)
    elif name == "seams":                                     # N = 3: foreground in the first and last rows and columns of every image
        lab = np.zeros((3, 24, 40), np.int32)
        for n in range(3):
            lab[n, :2, :] = 1
            lab[n, 22:, :] = 2
            _dumbbell(lab[n], 12, 6 + n, 30 + n, 5, 3)
            lab[n, 11:14, :8] = 3                             # the dumbbell reaches the row's first column
            lab[n, 8:16, 39] = 4
    elif name == "no_background":                             # image 0 has no label-0 pixel
        lab = np.concatenate([np.ones((1, 40, 64), np.int32), _two_discs()])
        lab[0, :, 32:] = 2
    elif name == "empty":
        lab = np.zeros((2, 20, 30), np.int32)
    elif name == "hand_tie":                                  # test_tie_by_hand's map, whose output is worked out there
        lab, p["ratio"] = np.ones((1, 3, 9), np.int32), (1, 2)
        lab[0, 0, 3:6] = lab[0, 2, 3:6] = 0
    elif name == "one_pixel":                                 # 1 x 1 foreground: an image with no background
        lab = np.ones((1, 1, 1), np.int32)
    elif name == "noise_drops":                               # many small cores: most are dropped, the slots run out
        lab, p = _noise(64, 96, 0.42, 99), dict(ratio=(1, 2), min_core=2, max_split=1, rows=16)
    elif name.startswith("noise"):
        _, H, W, dens = name.split("_")
        lab = _noise(int(H), int(W), int(dens) / 10, 7 * int(H) + int(W) + int(dens))
    elif name == "side_limit":                                # thick ends, a one-row neck between them, over the whole side
        S = _side_limit()
        lab = np.zeros((1, 3, S), np.int32)
        lab[0, 1, :] = 1
        lab[0, :, :60] = 1
        lab[0, :, S - 58:] = 1
    elif name == "out_of_range":                              # a label the call reads as background
        lab = _two_discs().copy()
        lab[0, :4, :4] = 1025
        lab[0, 36:, 60:] = -3
    else:
        raise KeyError(name)
    lab = np.ascontiguousarray(lab, np.int32)
    lab.setflags(write=False)
    return lab, p


SIZES = ["noise_1_1_5", "noise_1_1_7", "noise_1_70_5", "noise_1_70_7", "noise_70_1_5", "noise_70_1_7", "noise_33_33_5", "noise_33_33_7",
         "noise_45_70_5", "noise_45_70_7", "noise_64_96_5", "noise_64_96_7"]
CASES = ["two_discs", "two_discs_low_ratio", "bisector", "own_id", "concave", "core_drop_at", "core_drop_below", "core_drop_above", "core_drop_all",
         "slot_limit", "truncation", "diagonal_ids", "tile_corner", "seams", "no_background", "empty", "side_limit", "out_of_range", "one_pixel", "hand_tie", "noise_drops"] + SIZES


@functools.lru_cache(maxsize=None)
def want(name):
    lab, p = case(name)
    return R.split(lab, None, p["ratio"], p["min_core"], p["max_split"], p["rows"])


def _pred(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------

def test_the_restatements_distance_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    for name in ("two_discs", "concave", "noise_45_70_7", "seams", "tile_corner"):
        for lab in case(name)[0]:
            d = np.rint(ndi.distance_transform_edt(lab > 0) ** 2).astype(np.int64)
            assert np.array_equal(d, R.distance2(R.read_ids(lab))), name


def test_distance_by_hand():
    """A 3 x 5 map with background only at (0, 0):  D2(y, x) = y^2 + x^2 -- the image's edge is not background, so (2, 4) is 4 + 16
    away, not 1.  With no background at all there is no distance: -1."""
    lab = np.ones((3, 5), np.int64)
    lab[0, 0] = 0
    yy, xx = np.mgrid[:3, :5]
    assert np.array_equal(R.distance2(lab), yy * yy + xx * xx)
    assert (R.distance2(np.ones((3, 5), np.int64)) == -1).all()


def test_split_by_hand():
    """One row, id 1 on columns 1 .. 9, background at columns 0 and 10:
         D2 = 1 4 9 16 25 16 9 4 1, M2 = 25.  At 7/10 a core pixel needs 100 D2 > 49 * 25 = 1225, D2 >= 13: columns 4, 5, 6 -- ONE core,
         nothing is split.
       The same row with column 5 made background: two runs 1 .. 4 and 6 .. 9 of ONE id, D2 = 1 4 4 1 each, M2 = 4, core pixels
         100 D2 > 196: D2 = 4, columns 2, 3 and 7, 8 -- TWO cores.  The id is split: columns 1 .. 4 take the first core (new id 1), 6 .. 9
         the second (new id 2).  With min_core = 3 both cores are dropped and counted, and the id stays whole.
       Two such rows stacked with ids 1 and 2 and max_split = 1: id 1 is split into new ids 1, 2; id 2 qualifies, stays whole as
         new id 3 and is counted."""
    row = np.zeros((1, 11), np.int32)
    row[0, 1:10] = 1
    out, table, counts, info = R.split_image(row)
    assert info["d2"][0].tolist() == [0, 1, 4, 9, 16, 25, 16, 9, 4, 1, 0] and info["core"][0].tolist() == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert np.array_equal(out, row) and counts.tolist() == [1, 0, 0, 0] and table[0].tolist() == [9, 1, 0, 9, 0, 45, 0, 0]
    row[0, 5] = 0
    out, table, counts, info = R.split_image(row)
    assert info["core"][0].tolist() == [0, 0, 1, 1, 0, 0, 0, 2, 2, 0, 0] and out[0].tolist() == [0, 1, 1, 1, 1, 0, 2, 2, 2, 2, 0]
    assert counts.tolist() == [2, 1, 0, 0] and table[:2].tolist() == [[4, 1, 0, 4, 0, 10, 0, 0], [4, 6, 0, 9, 0, 30, 0, 0]]
    out, _, counts, _ = R.split_image(row, min_core=3)
    assert np.array_equal(out, row) and counts.tolist() == [1, 0, 2, 0]
    two = np.zeros((5, 11), np.int32)
    two[1], two[3] = row[0], row[0] * 2
    out, _, counts, _ = R.split_image(two, max_split=1)
    assert out[1].tolist() == [0, 1, 1, 1, 1, 0, 2, 2, 2, 2, 0] and out[3].tolist() == [0, 3, 3, 3, 3, 0, 3, 3, 3, 3, 0] and counts.tolist() == [3, 1, 0, 1]


def test_tie_by_hand():
    """A 3 x 9 map, id 1:   1 1 1 0 0 0 1 1 1      D2:   9 4 1 0 0 0 1 4 9      M2 = 10; at 1/2 a core pixel needs 4 D2 > 10, D2 >= 3:
                            1 1 1 1 1 1 1 1 1           10 5 2 1 1 1 2 5 10     columns 0, 1 are one core and columns 7, 8 the other.
                            1 1 1 0 0 0 1 1 1            9 4 1 0 0 0 1 4 9
    The neck's middle pixel (1, 4) is 9 away from the site (1, 1) and 9 away from the site (1, 7), and farther from every other:
    the smaller (y', x') wins, so it goes with the LEFT core, and the cut falls between columns 4 and 5."""
    lab = np.ones((3, 9), np.int32)
    lab[0, 3:6] = lab[2, 3:6] = 0
    out, _, counts, info = R.split_image(lab, ratio=(1, 2))
    assert info["d2"].tolist() == [[9, 4, 1, 0, 0, 0, 1, 4, 9], [10, 5, 2, 1, 1, 1, 2, 5, 10], [9, 4, 1, 0, 0, 0, 1, 4, 9]]
    assert (info["core"][:, :2] == 1).all() and (info["core"][:, 7:] == 2).all() and not info["core"][:, 2:7].any()
    assert counts.tolist() == [2, 1, 0, 0] and info["site"][1, 4] == 1 * 9 + 1
    assert out.tolist() == [[1, 1, 1, 0, 0, 0, 2, 2, 2], [1, 1, 1, 1, 1, 2, 2, 2, 2], [1, 1, 1, 0, 0, 0, 2, 2, 2]]
    assert np.array_equal(case("hand_tie")[0][0], lab) and want("hand_tie")["labels"][0].tolist() == out.tolist()      # the device runs this map too


# ---- CPU: every GPU input has the property it is named for ---------------------------------------------------------------------------

def _parts_of(name, n=0):
    w = want(name)
    return w["labels"][n], w["counts"][n].tolist(), w["info"][n]


def test_case_two_discs():
    lab, _ = case("two_discs")
    out, counts, info = _parts_of("two_discs")
    assert counts == [2, 1, 0, 0] and set(np.unique(out)) == {0, 1, 2} and np.array_equal(out > 0, lab[0] > 0)
    assert (out[:, :32][lab[0, :, :32] > 0] == 1).all() and (out[:, 33:][lab[0, :, 33:] > 0] == 2).all()
    out, counts, info = _parts_of("two_discs_low_ratio")
    assert counts == [1, 0, 0, 0] and len(info["kept"]) == 1 and np.array_equal(out, lab[0])


def test_case_bisector():
    """Every pixel of column 29 is as far from the left disc's core as from the right one's; the rule gives them to the left part."""
    lab, _ = case("bisector")
    out, counts, info = _parts_of("bisector")
    assert counts == [2, 1, 0, 0]
    sites = np.argwhere(info["core"] > 0)
    ties = 0
    for y in np.nonzero(lab[0, :, 29])[0]:
        d = (sites[:, 0] - y) ** 2 + (sites[:, 1] - 29) ** 2
        near = sites[d == d.min()]
        assert len(set(info["core"][tuple(s)] for s in near)) == 2
        ties += 1
        assert info["site"][y, 29] == min(s[0] * 60 + s[1] for s in near) and out[y, 29] == 1
    assert ties >= 3


def test_case_own_id():
    """Part of the dumbbell's bar is nearer to the blob's core than to either of its own; it still goes to its own."""
    lab, _ = case("own_id")
    out, counts, info = _parts_of("own_id")
    assert counts == [3, 1, 0, 0] and info["split"] == [1] and info["core_ids"].count(2) == 1
    sites = np.argwhere(info["core"] > 0)
    foreign = 0
    for y, x in np.argwhere(lab[0] == 1):
        d = (sites[:, 0] - y) ** 2 + (sites[:, 1] - x) ** 2
        if all(info["core_ids"][info["core"][tuple(s)] - 1] == 2 for s in sites[d == d.min()]):
            foreign += 1
    assert foreign >= 10
    assert set(np.unique(out[lab[0] == 1])) == {1, 2} and set(np.unique(out[lab[0] == 2])) == {3}


def test_case_concave():
    lab, _ = case("concave")
    out, counts, info = _parts_of("concave")
    assert counts == [2, 1, 0, 0] and components(lab[0] > 0, 8)[1] == 1
    assert max(components(out == 1, 8)[1], components(out == 2, 8)[1]) >= 2      # a cell in two pieces, held as defined


def test_case_core_drops():
    lab, _ = case("core_drop_at")
    areas = sorted(want("core_drop_at")["info"][0]["core_areas"])
    assert len(areas) == 2 and areas[0] < areas[1] and areas[0] >= 2
    assert [case("core_drop_" + k)[1]["min_core"] for k in ("below", "at", "above", "all")] == [areas[0] - 1, areas[0], areas[0] + 1, areas[1] + 1]
    assert _parts_of("core_drop_below")[1] == [2, 1, 0, 0] and _parts_of("core_drop_at")[1] == [2, 1, 0, 0]
    assert _parts_of("core_drop_above")[1] == [1, 0, 1, 0] and _parts_of("core_drop_all")[1] == [1, 0, 2, 0]
    assert np.array_equal(_parts_of("core_drop_all")[0], lab[0]) and np.array_equal(_parts_of("core_drop_above")[0], lab[0])


def test_case_slot_limit_and_truncation():
    lab, _ = case("slot_limit")
    out, counts, info = _parts_of("slot_limit")
    assert info["qualifying"] == [1, 2, 3] and info["split"] == [1, 2] and counts == [5, 2, 0, 1]
    assert set(np.unique(out[lab[0] == 3])) == {5} and set(np.unique(out[lab[0] == 2])) == {3, 4}
    w = want("truncation")
    assert w["counts"][0].tolist() == [6, 3, 0, 0] and w["table"].shape == (1, 3, 8) and (w["table"][0, :, 0] > 0).all() and w["labels"].max() == 6


def test_case_diagonal_ids():
    lab, _ = case("diagonal_ids")
    out, counts, info = _parts_of("diagonal_ids")
    assert np.array_equal(info["core"] > 0, lab[0] > 0)                           # every pixel is a core pixel
    assert lab[0, 2, 6] == 2 and lab[0, 3, 7] == 1 and lab[0, 3, 11] == 1 and lab[0, 4, 12] == 2      # the diagonal contacts
    assert components(lab[0] > 0, 8)[1] == 1 and components(lab[0] > 0, 4)[1] == 3
    assert info["core_ids"] == [2, 1, 2] and counts == [3, 1, 0, 0]               # joined across ids it would be one core and no split
    assert out[3, 7] == 1 and out[2, 2] == 2 and out[4, 16] == 3


def test_case_tile_corner():
    lab, _ = case("tile_corner")
    out, counts, info = _parts_of("tile_corner")
    assert counts == [4, 2, 0, 0] and lab[0, 32, 32] == 1 and info["core"][32, 32] == 0
    assert out[31, 31] != out[33, 33]                                             # the cut runs through the corner
    c = info["core"][32, 96]
    assert c > 0 and c == info["core"][31, 95] == info["core"][31, 96] == info["core"][32, 95]      # one core in four tiles


def test_case_seams():
    lab, _ = case("seams")
    assert (lab[:, 0] > 0).all() and (lab[:, -1] > 0).all() and (lab[:, 11:14, 0] > 0).all() and (lab[:, 8:16, -1] > 0).all()
    w = want("seams")
    assert (w["counts"][:, 1] == 1).all() and len({w["labels"][n].tobytes() for n in range(3)}) == 3


def test_case_no_background_and_empty():
    lab, _ = case("no_background")
    assert (lab[0] > 0).all()
    w = want("no_background")
    assert np.array_equal(w["labels"][0], lab[0]) and w["counts"].tolist() == [[2, 0, 0, 0], [2, 1, 0, 0]] and (w["info"][0]["d2"] == -1).all()
    w = want("empty")
    assert not w["labels"].any() and not w["table"].any() and not w["counts"].any()


def test_case_sizes_and_side_limit():
    assert sorted({tuple(case(n)[0].shape[1:]) for n in SIZES}) == [(1, 1), (1, 70), (33, 33), (45, 70), (64, 96), (70, 1)]
    for name in ("noise_33_33_5", "noise_33_33_7", "noise_45_70_5", "noise_45_70_7", "noise_64_96_5", "noise_64_96_7"):
        w = want(name)
        assert w["counts"][0, 1] >= 1 and w["counts"][0, 0] > case(name)[0].max(), name          # something is split
    assert want("one_pixel")["counts"].tolist() == [[1, 0, 0, 0]] and want("one_pixel")["labels"].tolist() == [[[1]]]
    K, split, dropped, whole = want("noise_drops")["counts"][0].tolist()
    assert split == 1 and dropped >= 10 and whole >= 1 and K > 16                                # cores dropped, slots run out, table truncated
    lab, _ = case("side_limit")
    S = _side_limit()
    from camouflage_multimodal_amd import _lib
    assert lab.shape == (1, 3, S) and S == _lib.SEG_WF_MAX_SIDE
    out, counts, info = _parts_of("side_limit")
    assert counts == [2, 1, 0, 0] and out[1, 0] == 1 and out[1, S - 1] == 2 and out[1, S // 2 - 2] == 1 and out[1, S // 2 + 2] == 2
    lab, _ = case("out_of_range")
    out, counts, _ = _parts_of("out_of_range")
    assert counts == [2, 1, 0, 0] and not out[:4, :4].any() and not out[36:, 60:].any()


# ---- CPU: the Python surface and the library's checks -----------------------------------------------------------------------------------

def test_python_argument_errors_by_name():
    from camouflage_multimodal_amd import _lib, split as S
    lab = torch.zeros(2, 8, 8, dtype=torch.int32)
    for kw, word in ((dict(ratio=0.7), "ratio"), (dict(ratio=(7, 7)), "ratio"), (dict(ratio=(0, 10)), "ratio"), (dict(ratio=(7, 17)), "ratio"),
                     (dict(ratio=(7.0, 10)), "ratio"), (dict(ratio=(True, 10)), "ratio"), (dict(ratio=(1, 2, 3)), "ratio"), (dict(min_core=-1), "min_core"),
                     (dict(min_core=1.5), "min_core"), (dict(max_split=0), "max_split"), (dict(max_split=9), "max_split"), (dict(max_split=True), "max_split"),
                     (dict(max_instances=0), "max_instances"), (dict(max_instances=_lib.INST_MAX_ROWS), "max_instances")):
        with pytest.raises(ValueError, match="^" + word):
            S.split_instances(lab, **kw)
    with pytest.raises(ValueError, match="^labels must be int32"):
        S.split_instances(lab.long())
    with pytest.raises(ValueError, match="^labels must be a tensor"):
        S.split_instances(lab.numpy())
    with pytest.raises(ValueError, match="^need labels"):
        S.split_instances(torch.zeros(0, 8, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="^need pred of labels' shape"):
        S.split_instances(lab, torch.zeros(2, 8, 9))
    with pytest.raises(ValueError, match="^pred must be a tensor"):
        S.split_instances(lab, np.zeros((2, 8, 8), np.float32))
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        S.split_instances(lab)
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        S.split_instances(lab, torch.zeros(2, 8, 8))


def test_split_options():
    from camouflage_multimodal_amd import split as S
    assert S.split_options(None) is None and S.split_options(False) is None and S.split_options(False, instances=False) is None
    assert S.split_options(True) == {"ratio": (7, 10), "min_core": 0, "max_split": 4, "max_instances": 64}
    assert S.split_options({"ratio": [1, 2], "max_split": 8}) == {"ratio": (1, 2), "min_core": 0, "max_split": 8, "max_instances": 64}
    with pytest.raises(ValueError, match="^split needs instances=True"):
        S.split_options(True, instances=False)
    for bad in (1, "yes", {"radius": 3}, [7, 10]):
        with pytest.raises(ValueError, match="^split must be"):
            S.split_options(bad)
    with pytest.raises(ValueError, match="^max_split"):
        S.split_options({"max_split": 9})
    with pytest.raises(ValueError, match="^ratio"):
        S.split_options({"ratio": (10, 7)})


def test_split_records_on_the_host():
    from camouflage_multimodal_amd import split as S
    w = want("slot_limit")
    rec, = S.split_records(torch.from_numpy(w["table"]), torch.from_numpy(w["counts"]), 48, 32)
    assert rec["count"] == 5 and rec["split"] == 2 and rec["cores_dropped"] == 0 and rec["left_whole"] == 1 and not rec["truncated"]
    assert [i["id"] for i in rec["instances"]] == [1, 2, 3, 4, 5] and all(i["score"] == 0.0 for i in rec["instances"])
    assert rec["instances"][0]["area"] == int((w["labels"][0] == 1).sum())
    w = want("truncation")
    rec, = S.split_records(w["table"].tolist(), w["counts"].tolist(), 48, 32)
    assert rec["count"] == 6 and rec["truncated"] and len(rec["instances"]) == 3
    with pytest.raises(ValueError, match="counts rows"):
        S.split_records(w["table"].tolist(), [[1, 2, 3]], 48, 32)


def test_header_constants_and_symbols():
    from camouflage_multimodal_amd import _lib
    raw = open(os.path.join(ROOT, "include", "camo_split.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    assert int(m["CAMO_SPLIT_MAX_SPLIT"]) == _lib.SPLIT_MAX_SPLIT == 8 and int(m["CAMO_SPLIT_MAX_DEN"]) == _lib.SPLIT_MAX_DEN == 16
    assert int(m["CAMO_SPLIT_COUNTS"]) == _lib.SPLIT_COUNTS == R.COUNTS and _lib.IM_MAX_IDS == R.MAX_ID
    src = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "split.hip")).read()
    launcher = src.split("int launch_split(")[1]
    assert int(m["CAMO_SPLIT_LAUNCHES"]) == _lib.SPLIT_LAUNCHES == launcher.count("hipLaunchKernelGGL(")
    assert not re.search(r"\b(for|while|if)\b", launcher.split("{", 1)[1])        # the launches depend on nothing
    assert "hipMalloc" not in src and "Synchronize" not in src and not re.search(r"atomic(Add|Min|Max|CAS)\s*\(\s*\(?\s*(float|double)", src)
    assert "PARITY UNPINNED" in raw and "Not built" in raw and _lib.ABI_VERSION == 13
    assert _lib.symbols("camo_split.h") == ("camo_split_workspace_bytes", "camo_split_instances")


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L, S = _lib.lib(), _side_limit()
    ws = L.camo_split_workspace_bytes
    assert ws(1, 1, 1, 1) > 0 and ws(1, 1, 1, 1) % 256 == 0 and ws(2, 45, 70, 8) > ws(2, 45, 70, 4) > ws(1, 45, 70, 4) and ws(1, 3, S, 4) > 0 and ws(1, S, S, 8) > 0
    for bad in ((0, 8, 8, 4), (65536, 1, 1, 4), (1, 0, 8, 4), (1, 8, -1, 4), (1, S + 1, 8, 4), (1, 8, S + 1, 4), (257, S, S, 4), (1, 8, 8, 0), (1, 8, 8, 9), (1, 8, 8, -1)):
        assert ws(*bad) == 0, bad
    p, q, big = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), 1 << 40
    good = dict(labels=p, pred=None, stride=0, N=2, H=8, W=8, num=7, den=10, min_core=0, max_split=4, rows=64, out=q, table=ctypes.c_void_p(0x300000),
                counts=ctypes.c_void_p(0x400000), ws=ctypes.c_void_p(0x500000), nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return L.camo_split_instances(a["labels"], a["pred"], a["stride"], a["N"], a["H"], a["W"], a["num"], a["den"], a["min_core"], a["max_split"], a["rows"],
                                      a["out"], a["table"], a["counts"], a["ws"], a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=S + 1), dict(W=S + 1), dict(num=0), dict(num=10), dict(num=11), dict(den=17), dict(den=1, num=1),
               dict(num=-7, den=-10), dict(min_core=-1), dict(max_split=0), dict(max_split=9), dict(rows=0), dict(rows=_lib.INST_MAX_ROWS), dict(pred=p, stride=63),
               dict(pred=p, stride=-1), dict(labels=None), dict(out=None), dict(table=None), dict(counts=None), dict(ws=None), dict(out=p),
               dict(out=ctypes.c_void_p(0x100000 + 2 * 8 * 8 * 4 - 4)), dict(labels=ctypes.c_void_p(0x200000 + 4)), dict(table=ctypes.c_void_p(0x300004)),
               dict(ws=ctypes.c_void_p(0x500080)), dict(nbytes=ws(2, 8, 8, 4) - 1), dict(nbytes=0)):
        assert call(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def split_call(lab, pred=None, channel=0, ratio=(7, 10), min_core=0, max_split=4, rows=64):
    """camo_split_instances as a raw_calls.Call.  ``pred``: None, fp32 [N, H, W], or fp32 [N, C, H, W] whose ``channel`` is read in place."""
    from camouflage_multimodal_amd import _lib
    L, (N, H, W) = _lib.lib(), lab.shape
    at, stride, ins = 0, 0, {"labels": np.asarray(lab, np.int32)}
    if pred is not None:
        ins["pred"] = pred = np.asarray(pred, np.float32)
        at, stride = (4 * channel * H * W, pred.shape[1] * H * W) if pred.ndim == 4 else (0, H * W)
    nbytes = L.camo_split_workspace_bytes(N, H, W, max_split)
    assert nbytes > 0 and nbytes % 256 == 0
    outs = {"labels_out": ((N, H, W), np.int32), "table": ((N, rows, 8), np.int64), "counts": ((N, 4), np.int32)}
    return Call(outs, nbytes, lambda p, w, nb: L.camo_split_instances(p["labels"], p["pred"] + at if pred is not None else None, stride, N, H, W, ratio[0], ratio[1],
                                                                      min_core, max_split, rows, p["labels_out"], p["table"], p["counts"], w, nb,
                                                                      torch.cuda.current_stream().cuda_stream), ins)


def _run(lab, pred=None, channel=0, fill=0xA5, ws_fill=0xFF, before=(), **p):
    got = execute(split_call(lab, pred, channel, **p), fill, before=before, ws_fill=ws_fill, skew=8)
    return {"labels": got["labels_out"], "table": got["table"], "counts": got["counts"]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_split_equals_the_restatement_bytewise(name):
    lab, p = case(name)
    same_bytes(_run(lab, **p), want(name), name, NAMES)


@pytest.mark.gpu
def test_split_on_workspace_of_every_fill_and_after_a_larger_call():
    lab, p = case("seams")
    for fill, ws_fill in ((0x00, 0x00), (0xFF, 0x7F), (0x7F, 0xA5)):
        same_bytes(_run(lab, fill=fill, ws_fill=ws_fill, **p), want("seams"), (fill, ws_fill), NAMES)
    larger = split_call(np.ascontiguousarray(lab[::-1]), **dict(p, max_split=8, ratio=(1, 2)))      # (more workspace, other contents)
    assert larger.ws > split_call(lab, **p).ws
    same_bytes(_run(lab, before=(larger,), **p), want("seams"), "after a larger call", NAMES)


@pytest.mark.gpu
def test_sq_with_and_without_pred():
    lab, p = case("seams")
    pred = _pred(lab.shape, 3)
    pred[0, 0, :3] = (np.nan, -2.0, 7.0)
    ref = R.split(lab, pred, p["ratio"], p["min_core"], p["max_split"], p["rows"])
    got = _run(lab, pred, **p)
    same_bytes(got, ref, "with pred", NAMES)
    assert (got["table"][..., 7] > 0).any() and not want("seams")["table"][..., 7].any()
    same_bytes(_run(lab, **p), want("seams"), "pred null", NAMES)


@pytest.mark.gpu
def test_pred_channel_is_read_in_place():
    lab, p = case("seams")
    maps = _pred((3, 3) + lab.shape[1:], 5)
    ref = R.split(lab, maps[:, 1], p["ratio"], p["min_core"], p["max_split"], p["rows"])
    same_bytes(_run(lab, maps, 1, **p), ref, "channel 1", NAMES)
    assert ref["table"].tobytes() != R.split(lab, maps[:, 0], p["ratio"], p["min_core"], p["max_split"], p["rows"])["table"].tobytes()


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_agree():
    maps = [case(n)[0][0] for n in ("two_discs", "core_drop_at")] + [np.ascontiguousarray(case("two_discs")[0][0, ::-1])]
    batch = np.stack(maps)
    pred = _pred(batch.shape, 11)
    whole = _run(batch, pred)
    again = _run(batch, pred, fill=0x00, ws_fill=0x00)
    same_bytes(again, whole, "two calls", NAMES)
    for n in range(3):
        one = _run(batch[n:n + 1], pred[n:n + 1])
        same_bytes({k: v[0] for k, v in one.items()}, {k: v[n] for k, v in whole.items()}, n, NAMES)
    same_bytes(whole, R.split(batch, pred), "the batch", NAMES)


@pytest.mark.gpu
def test_python_surface_on_the_device():
    from camouflage_multimodal_amd import split as S
    lab, p = case("slot_limit")
    t = torch.from_numpy(np.array(lab)).cuda()
    out = S.split_instances(t, None, p["ratio"], p["min_core"], p["max_split"], p["rows"])
    same_bytes({k: v.cpu().numpy() for k, v in out.items()}, want("slot_limit"), "split_instances", NAMES)
    one = S.split_instances(t[0], max_split=2)
    assert tuple(one["labels"].shape) == (1, 48, 32) and torch.equal(one["labels"], out["labels"])
    rec, = S.split_records(out["table"], out["counts"], 48, 32)
    assert rec["count"] == 5 and rec["split"] == 2 and rec["left_whole"] == 1 and len(rec["instances"]) == 5
    found = S.split_detected(t, None, S.split_options({"max_instances": 2}))
    assert found["table"].shape[1] == 6 and not found["instances"][0]["truncated"] and found["instances"][0]["count"] == 6
    pred = torch.from_numpy(_pred((1, 3, 48, 32), 2)).cuda()
    ref = R.split(lab, pred[:, 2].cpu().numpy())
    same_bytes({k: v.cpu().numpy() for k, v in S.split_instances(t, pred[:, 2]).items()}, ref, "a channel view", NAMES)
