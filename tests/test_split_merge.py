"""Low-dynamic cores merged (include/camo_split_merge.h): camo_split_merge against tests/split_merge_ref.py, byte for byte.

CPU: the restatement's hand cases, every ValueError and CamoError of ``split.merge_parts``, the library's argument checks with pointers
that are never dereferenced, the workspace query, the constants, and -- for every input of the GPU tests -- a test that shows from the
restatement alone that the input has the property it is named for.  GPU: every buffer of every call sits between guards on memory the
call did not clear (tests/guarded.py, tests/raw_calls.py, the call stated in tests/split_merge_calls.py) and is compared byte for byte.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import split_geo_ref as G
import split_merge_ref as M
import split_ref as R
from conftest import ROOT
from instances_ref import components
from raw_calls import same_bytes
from split_merge_calls import NAMES, merge_call, run


def _disc(lab, cy, cx, r, value=1):
    yy, xx = np.mgrid[:lab.shape[0], :lab.shape[1]]
    lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value


def _discs(H, W, *discs):
    lab = np.zeros((H, W), np.int32)
    for d in discs:
        _disc(lab, *d)
    return lab


def _noise(H, W, percent, seed):
    lab, n = components(np.random.RandomState(seed).rand(H, W) < percent / 100, 8)
    assert n <= R.MAX_ID
    return lab.astype(np.int32)


def _neck(rows):
    """Two bodies 39 x 39 joined by a neck of ``rows`` rows and 40 columns, one id; the parts are cut at column 60, inside the neck."""
    lab = np.zeros((41, 120), np.int32)
    lab[1:40, 1:40] = lab[1:40, 80:119] = 1
    top = 20 - rows // 2
    lab[top:top + rows, 40:80] = 1
    return lab, (np.where(np.arange(120)[None] < 60, 1, 2) * (lab > 0)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (labels int32 [N, H, W], parts int32 [N, H, W], merge, rows).  Read-only: the arrays are shared."""
    merge, rows = (4, 5), 64
    if name.startswith("lobe"):                               # lobe_<euclid|geo>_<num>_<den>
        _, growth, num, den = name.split("_")
        lab = _discs(64, 120, (30, 22, 20), (30, 56, 20), (30, 80, 15))
        parts, merge = (R if growth == "euclid" else G).split_image(lab, ratio=(7, 10))[0], (int(num), int(den))
    elif name.startswith("chain") or name.startswith("gaps"):  # three equal discs in a row: peaks 101, contacts 49
        kind, num, den = name.split("_")
        lab = _discs(40, 64, (20, 12, 10), (20, 28, 10), (20, 44, 10))
        parts, merge = R.split_image(lab, ratio=(8, 10))[0], (int(num), int(den))
        if kind == "gaps":
            parts = np.array([0, 2, 5, 9], np.int32)[parts]
    elif name == "bridge":
        lab = _discs(64, 128, (30, 22, 20), (30, 102, 20), (30, 62, 15))
        lab[18:43, 22:103] = 1
        parts = R.split_image(lab, ratio=(7, 10))[0]
    elif name.startswith("neck"):
        lab, parts = _neck(int(name.split("_")[1]))
    elif name == "two_ids":                                    # ids 1 and 2 side by side, a part each
        lab = np.zeros((12, 24), np.int32)
        lab[2:10, 2:12], lab[2:10, 12:22] = 1, 2
        parts, merge = lab.copy(), (1, 16)
    elif name == "diagonal":                                   # one-pixel bars of one id: part 2 meets part 1 to its NW and part 3 to its NE
        lab = np.zeros((6, 20), np.int32)
        lab[2, 2:7] = lab[3, 7:12] = lab[2, 12:17] = 1
        parts = np.zeros_like(lab)
        parts[2, 2:7], parts[3, 7:12], parts[2, 12:17] = 1, 2, 3
        merge = (1, 1)
    elif name == "tile_corner":                                # two squares of one id that meet at (31, 31) | (32, 32) only
        lab = np.zeros((64, 64), np.int32)
        lab[24:32, 24:32] = lab[32:40, 32:40] = 1
        parts = lab.copy()
        parts[32:40, 32:40] = 2
        merge = (1, 4)
    elif name == "seam":                                       # W = 70: pixel 1024 is (14, 44); the cut between rows 14 and 15 crosses it
        lab = np.zeros((40, 70), np.int32)
        lab[4:31, 4:66] = 1
        parts = lab.copy()
        parts[15:] *= 2
        merge = (1, 2)
    elif name == "many":                                       # 32 x 32, every pixel a part of its own: 1024 parts, no background
        lab = np.ones((32, 32), np.int32)
        parts = np.arange(1, 1025, dtype=np.int32).reshape(32, 32)
    elif name == "deep":                                       # one row of 1024 one-pixel parts with equal peaks: part a joins a - 1, a chain 1023 long
        lab = np.zeros((3, 1026), np.int32)
        lab[1, 1:1025] = 1
        parts, merge, rows = (lab * np.arange(1026)[None]).astype(np.int32), (1, 1), 4
    elif name == "bad_part":                                   # N = 3: image 1 holds the part value 1025 on a foreground pixel
        lab, parts, merge, rows = case("chain_3_5")
        lab, parts = np.repeat(lab, 3, 0), np.repeat(parts, 3, 0)
        parts[1, 20, 12] = 1025
        parts[2][parts[2] == 3] = 1024
    elif name == "no_background":
        lab = np.ones((8, 8), np.int32)
        parts = lab.copy()
        parts[:, 4:] = 2
        merge = (1, 16)
    elif name == "empty":
        lab = np.zeros((2, 20, 30), np.int32)
        parts = np.full((2, 20, 30), 7, np.int32)              # (what parts holds on the background is not read)
    elif name == "truncation":
        lab, parts, merge, _ = case("lobe_euclid_4_5")
        rows = 1
    elif name.startswith("noise"):                             # noise_<H>_<W>_<percent>
        _, H, W, percent = name.split("_")
        lab = _noise(int(H), int(W), int(percent), 1)
        parts, merge = R.split_image(lab, ratio=(3, 10), max_split=8)[0], (1, 2)
    else:
        raise KeyError(name)
    lab, parts = (np.ascontiguousarray(a if a.ndim == 3 else a[None], np.int32) for a in (lab, parts))
    lab.setflags(write=False)
    parts.setflags(write=False)
    return lab, parts, merge, rows


SIZES = ["noise_1_1_80", "noise_1_70_80", "noise_70_1_80", "noise_33_33_80", "noise_45_70_80", "noise_45_70_90"]
CASES = ["lobe_euclid_4_5", "lobe_euclid_9_10", "lobe_geo_4_5", "lobe_geo_9_10", "chain_3_5", "chain_15_16", "bridge", "neck_31", "neck_29", "two_ids",
         "diagonal", "tile_corner", "seam", "gaps_3_5", "gaps_15_16", "many", "deep", "bad_part", "no_background", "empty", "truncation"] + SIZES


@functools.lru_cache(maxsize=None)
def want(name):
    lab, parts, merge, rows = case(name)
    return M.merge(lab, parts, None, merge, rows)


def _of(name, n=0):
    w = want(name)
    return w["labels"][n], w["counts"][n].tolist(), w["info"][n]


def _pred(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


# ---- CPU: the restatement by hand ---------------------------------------------------------------------------------------------------

def test_one_row_by_hand():
    """One row, id 1 on columns 1 .. 9, background at columns 0 and 10:  D2 = 1 4 9 16 25 16 9 4 1.
    Parts 1 1 1 2 2 2 2 3 3: peaks 9, 25, 4, so part 2 is the highest, then 1, then 3.  The contact 1|2 at columns 3|4 is
    min(9, 16) = 9 and the contact 2|3 at columns 7|8 is min(9, 4) = 4: pass(1) = 9 = peak(1) and pass(3) = 4 = peak(3), so both are
    linked even at 1/1.  One group: K'' = 1, three part ids, one group of several, and id 1 is whole again.
    Parts 1 1 1 1 1 2 2 2 2, cut beside the peak: the contact is min(25, 16) = 16, part 2's whole height."""
    lab = np.zeros((1, 11), np.int32)
    lab[0, 1:10] = 1
    parts = np.array([[0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 0]], np.int32)
    out, table, counts, info = M.merge_image(lab, parts, None, (1, 1))
    assert info["d2"][0].tolist() == [0, 1, 4, 9, 16, 25, 16, 9, 4, 1, 0] and info["peak"] == {1: 9, 2: 25, 3: 4}
    assert info["contacts"] == {(1, 2): 9, (3, 2): 4} and info["links"] == {1: 2, 3: 2}
    assert out.tolist() == lab.tolist() and counts.tolist() == [1, 3, 1, 1] and table[0].tolist() == [9, 1, 0, 9, 0, 45, 0, 0]
    parts = np.array([[0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 0]], np.int32)
    assert M.merge_image(lab, parts, None, (1, 1))[3]["contacts"] == {(2, 1): 16}


def test_equal_peaks_and_two_ids_by_hand():
    """Rows 1 and 3 of a 5 x 11 map hold ids 1 and 2 on columns 1 .. 9, with background rows around them: every D2 is 1.  Id 1 is
    cut into parts 1 | 2 and id 2 into parts 3 | 4.  All peaks are 1, so the smaller part id is the higher one: 2 -> 1 and 4 -> 3
    across contacts of value 1, which is the peak itself: linked at 1/1.  The ids never meet (a background row lies between), the
    groups are {1, 2} and {3, 4}, and the output is the input map: both ids are whole again."""
    lab = np.zeros((5, 11), np.int32)
    lab[1, 1:10], lab[3, 1:10] = 1, 2
    parts = np.zeros_like(lab)
    parts[1, 1:4], parts[1, 4:10], parts[3, 1:3], parts[3, 3:10] = 1, 2, 3, 4
    out, _, counts, info = M.merge_image(lab, parts, None, (1, 1))
    assert (info["d2"][[1, 3], 1:10] == 1).all() and info["peak"] == {1: 1, 2: 1, 3: 1, 4: 1}
    assert info["contacts"] == {(2, 1): 1, (4, 3): 1} and info["links"] == {2: 1, 4: 3} and counts.tolist() == [2, 4, 2, 2] and np.array_equal(out, lab)
    assert M.higher(5, 6, {5: 1, 6: 1}) and not M.higher(6, 5, {5: 1, 6: 1}) and M.higher(6, 5, {5: 1, 6: 2})


def test_unsupported_by_hand():
    lab = np.array([[1, 1, 0, 3000]], np.int32)
    out, table, counts, info = M.merge_image(lab, np.array([[1, 1025, 9, 9]], np.int32))
    assert out.tolist() == [[1, 1025, 0, 0]] and counts.tolist() == [-1, 0, 0, 0] and not table.any() and not info["supported"]
    out, _, counts, _ = M.merge_image(lab, np.array([[4, 4, -5, 2000]], np.int32))      # a bad value where labels reads 0 is not read
    assert out.tolist() == [[1, 1, 0, 0]] and counts.tolist() == [1, 1, 0, 0]
    assert M.merge_image(lab, np.array([[0, 1, 0, 0]], np.int32))[2].tolist() == [-1, 0, 0, 0]


# ---- CPU: every GPU input has the property it is named for ---------------------------------------------------------------------------

@pytest.mark.parametrize("growth", ["euclid", "geo"])
def test_case_lobe(growth):
    """Peaks 401, 401, 226; the lobe's contact with its body is 169, the true neck's 121.  25 * 169 = 4225 >= 16 * 226 = 3616 links
    3 -> 2; 25 * 121 = 3025 < 16 * 401 = 6416 leaves the neck.  At 9/10, 100 * 169 = 16900 < 81 * 226 = 18306: nothing links."""
    lab, parts, _, _ = case(f"lobe_{growth}_4_5")
    out, counts, info = _of(f"lobe_{growth}_4_5")
    assert info["peak"] == {1: 401, 2: 401, 3: 226} and info["contacts"] == {(3, 2): 169, (2, 1): 121}
    assert info["links"] == {3: 2} and counts == [2, 3, 1, 0]
    assert sorted(np.bincount(out.ravel())[1:].tolist()) == [1226, 1722]
    out, counts, info = _of(f"lobe_{growth}_9_10")
    assert info["links"] == {} and counts == [3, 3, 0, 0] and np.array_equal(out, parts[0])
    assert 25 * 169 >= 16 * 226 and 25 * 121 < 16 * 401 and 100 * 169 < 81 * 226


def test_case_chain_and_gaps():
    """Peaks 101 each, contacts 49: 25 * 49 = 1225 >= 9 * 101 = 909 links 2 -> 1 and 3 -> 2; 256 * 49 < 225 * 101 links nothing."""
    out, counts, info = _of("chain_3_5")
    assert info["peak"] == {1: 101, 2: 101, 3: 101} and info["contacts"] == {(2, 1): 49, (3, 2): 49}
    assert info["links"] == {2: 1, 3: 2} and counts == [1, 3, 1, 1] and np.array_equal(out, case("chain_3_5")[0][0])
    out, counts, info = _of("chain_15_16")
    assert info["links"] == {} and counts == [3, 3, 0, 0] and np.array_equal(out, case("chain_15_16")[1][0])
    assert sorted(np.unique(case("gaps_3_5")[1])) == [0, 2, 5, 9]
    out, counts, info = _of("gaps_15_16")
    assert counts == [3, 3, 0, 0] and info["new_of"] == {2: 1, 5: 2, 9: 3} and np.array_equal(out, case("chain_15_16")[1][0])      # the gaps closed
    assert _of("gaps_3_5")[1] == [1, 3, 1, 1] and _of("gaps_3_5")[2]["links"] == {5: 2, 9: 5}


def test_case_bridge():
    """Part 3 has contacts of 169 with both bodies; the tie goes to part 1, and the two bodies stay apart: K'' = 2, not 1."""
    out, counts, info = _of("bridge")
    assert info["peak"] == {1: 401, 2: 401, 3: 226} and info["contacts"] == {(3, 1): 169, (3, 2): 169}
    assert info["pass"] == {3: (169, 1)} and info["links"] == {3: 1} and counts == [2, 3, 1, 0]
    assert info["new_of"] == {1: 1, 3: 1, 2: 2}


def test_case_equality():
    """A neck 31 rows tall: contact 16^2 = 256, 25 * 256 = 6400 = 16 * 400: linked.  29 rows: 15^2 = 225, 5625 < 6400: not linked."""
    out, counts, info = _of("neck_31")
    assert info["peak"] == {1: 400, 2: 400} and info["contacts"] == {(2, 1): 256} and info["links"] == {2: 1} and counts == [1, 2, 1, 1]
    out, counts, info = _of("neck_29")
    assert info["peak"] == {1: 400, 2: 400} and info["contacts"] == {(2, 1): 225} and info["links"] == {} and counts == [2, 2, 0, 0]
    assert 25 * 256 == 16 * 400 and 25 * 225 < 16 * 400


def test_case_contact_geometry():
    lab, parts, merge, _ = case("two_ids")
    out, counts, info = _of("two_ids")
    assert merge == (1, 16) and (lab[0, :, 11] == 1).sum() == 8 and (lab[0, :, 12] == 2).sum() == 8      # they touch along a column
    assert info["contacts"] == {} and counts == [2, 2, 0, 0]
    lab, parts, _, _ = case("diagonal")
    out, counts, info = _of("diagonal")
    assert parts[0, 2, 6] == 1 and parts[0, 3, 7] == 2 and parts[0, 3, 11] == 2 and parts[0, 2, 12] == 3      # SE of part 1's end, SW of part 3's start
    assert components(lab[0] > 0, 4)[1] == 3 and components(lab[0] > 0, 8)[1] == 1
    assert info["contacts"] == {(2, 1): 1, (3, 2): 1} and info["links"] == {2: 1, 3: 2} and counts == [1, 3, 1, 1]
    lab, parts, _, _ = case("tile_corner")
    out, counts, info = _of("tile_corner")
    assert parts[0, 31, 31] == 1 and parts[0, 32, 32] == 2 and lab[0, 31, 32] == 0 and lab[0, 32, 31] == 0
    assert info["peak"] == {1: 16, 2: 16} and info["contacts"] == {(2, 1): 1} and info["links"] == {2: 1} and counts == [1, 2, 1, 1]      # 16 * 1 >= 1 * 16
    lab, parts, _, _ = case("seam")
    out, counts, info = _of("seam")
    W = lab.shape[2]
    assert 14 * W + 44 == 1024 and parts[0, 14, 43] == 1 and parts[0, 15, 42] == 2 and parts[0, 14, 44] == 1 and parts[0, 15, 45] == 2
    assert len(info["contacts"]) == 1 and len(info["links"]) == 1 and counts == [1, 2, 1, 1]


def test_case_part_ids():
    lab, parts, _, _ = case("many")
    out, counts, info = _of("many")
    assert lab.shape == (1, 32, 32) and len(np.unique(parts)) == 1024 and parts.max() == 1024
    assert counts == [1024, 1024, 0, 0] and np.array_equal(out, parts[0]) and (info["d2"] == -1).all()
    out, counts, info = _of("deep")
    assert len(info["links"]) == 1023 and all(b == a - 1 for a, b in info["links"].items()) and counts == [1, 1024, 1, 1]
    lab, parts, _, _ = case("bad_part")
    w = want("bad_part")
    assert w["counts"].tolist() == [[1, 3, 1, 1], [-1, 0, 0, 0], [1, 3, 1, 1]] and not w["table"][1].any() and w["table"][0, 0, 0] > 0
    assert np.array_equal(w["labels"][1], parts[1]) and w["labels"][1].max() == 1025 and np.array_equal(w["labels"][0], w["labels"][2])


def test_case_sizes_and_backgrounds():
    lab, parts, merge, _ = case("no_background")
    out, counts, info = _of("no_background")
    assert (lab > 0).all() and merge == (1, 16) and counts == [2, 2, 0, 0] and np.array_equal(out, parts[0]) and info["contacts"] == {}
    w = want("empty")
    assert not w["labels"].any() and not w["table"].any() and not w["counts"].any()
    assert sorted({tuple(case(n)[0].shape[1:]) for n in SIZES}) == [(1, 1), (1, 70), (33, 33), (45, 70), (70, 1)]
    w = want("truncation")
    assert w["table"].shape == (1, 1, 8) and w["counts"][0, 0] == 2 and w["table"][0, 0, 0] == 1226


@pytest.mark.parametrize("name", ["noise_45_70_80", "noise_45_70_90"])
def test_case_noise_links_and_does_not_link(name):
    out, counts, info = _of(name)
    unlinked = [a for a in info["pass"] if a not in info["links"]]
    assert len(info["links"]) >= 1 and len(unlinked) >= 1, (len(info["links"]), len(unlinked))
    assert counts[1] > counts[0] and counts[2] >= 1


# ---- CPU: the Python surface and the library's checks -----------------------------------------------------------------------------------

def test_python_argument_errors_by_name():
    from camouflage_multimodal_amd import _lib, split as S
    lab = torch.zeros(2, 8, 8, dtype=torch.int32)
    for kw, word in ((dict(merge=0.8), "merge"), (dict(merge=(5, 4)), "merge"), (dict(merge=(0, 5)), "merge"), (dict(merge=(4, 17)), "merge"),
                     (dict(merge=(4.0, 5)), "merge"), (dict(merge=(True, 5)), "merge"), (dict(merge=(1, 2, 3)), "merge"), (dict(merge=None), "merge"),
                     (dict(max_instances=0), "max_instances"), (dict(max_instances=1.5), "max_instances"), (dict(max_instances=_lib.INST_MAX_ROWS), "max_instances")):
        with pytest.raises(ValueError, match="^" + word):
            S.merge_parts(lab, lab, **kw)
    assert S.check_merge((5, 5)) == (5, 5) and S.check_merge([4, 5]) == (4, 5)
    with pytest.raises(ValueError, match="^merge"):
        S.split_instances(lab, merge=(5, 4))
    with pytest.raises(ValueError, match="^labels must be int32"):
        S.merge_parts(lab.long(), lab)
    with pytest.raises(ValueError, match="^parts must be int32"):
        S.merge_parts(lab, lab.long())
    with pytest.raises(ValueError, match="^parts must be a tensor"):
        S.merge_parts(lab, lab.numpy())
    with pytest.raises(ValueError, match="^need parts of labels' shape"):
        S.merge_parts(lab, torch.zeros(2, 8, 9, dtype=torch.int32))
    with pytest.raises(ValueError, match="^need pred of labels' shape"):
        S.merge_parts(lab, lab, torch.zeros(2, 8, 9))
    with pytest.raises(ValueError, match="^pred must be a tensor"):
        S.merge_parts(lab, lab, np.zeros((2, 8, 8), np.float32))
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        S.merge_parts(lab, lab)
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        S.split_instances(lab, merge=(4, 5))


def test_split_options_take_merge():
    from camouflage_multimodal_amd import split as S
    base = {"ratio": (7, 10), "min_core": 0, "max_split": 4, "max_instances": 64}
    assert S.split_options({"merge": [4, 5]}) == {**base, "merge": (4, 5)} and S.split_options({"merge": None}) == base == S.split_options(True)
    for bad in ((5, 4), 0.8, (4, 5, 6), True):
        with pytest.raises(ValueError, match="^merge"):
            S.split_options({"merge": bad})
    with pytest.raises(ValueError, match="^split must be"):
        S.split_options({"merged": (4, 5)})
    with pytest.raises(ValueError, match="^split needs instances=True"):
        S.split_options({"merge": (4, 5)}, instances=False)
    with pytest.raises(ValueError, match="^max_split"):
        S.split_options({"merge": (4, 5), "max_split": 9})


def test_split_records_with_merge_counts():
    from camouflage_multimodal_amd import split as S
    w = want("lobe_euclid_4_5")
    split_counts = [[3, 1, 0, 0]]
    rec, = S.split_records(torch.from_numpy(w["table"]), torch.tensor(split_counts, dtype=torch.int32), 64, 120, torch.from_numpy(w["counts"]))
    assert rec["count"] == 2 and rec["split"] == 1 and rec["parts"] == 3 and rec["merged_groups"] == 1 and rec["made_whole"] == 0 and not rec["truncated"]
    assert [i["area"] for i in rec["instances"]] == [1226, 1722]
    plain, = S.split_records(w["table"].tolist(), [[2, 1, 0, 0]], 64, 120)                     # (without them: today's keys, the count from counts)
    assert sorted(set(rec) - set(plain)) == ["made_whole", "merged_groups", "parts"] and plain["count"] == 2
    t = want("truncation")
    rec, = S.split_records(t["table"].tolist(), split_counts, 64, 120, t["counts"].tolist())
    assert rec["count"] == 2 and rec["truncated"] and len(rec["instances"]) == 1
    with pytest.raises(ValueError, match="merge_counts rows"):
        S.split_records(w["table"].tolist(), split_counts, 64, 120, [[1, 2, 3]])
    with pytest.raises(ValueError, match="^merge_counts holds 2 images"):
        S.split_records(w["table"].tolist(), split_counts, 64, 120, [[2, 3, 1, 0]] * 2)


def test_header_constants_and_symbols():
    from camouflage_multimodal_amd import _lib
    raw = open(os.path.join(ROOT, "include", "camo_split_merge.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    assert int(m["CAMO_SPLIT_MERGE_COUNTS"]) == _lib.SPLIT_MERGE_COUNTS == M.COUNTS == 4
    src = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "split_merge.hip")).read()
    launcher = src.split("int launch_split_merge(")[1]
    assert int(m["CAMO_SPLIT_MERGE_LAUNCHES"]) == _lib.SPLIT_MERGE_LAUNCHES == launcher.count("hipLaunchKernelGGL(")
    assert not re.search(r"\b(for|while|if)\b", launcher.split("{", 1)[1])        # the launches depend on nothing
    assert "hipMalloc" not in src and "Synchronize" not in src and not re.search(r"atomic(Add|Min|Max|CAS)\s*\(\s*\(?\s*(float|double)", src)
    assert "PARITY UNPINNED" in raw and "Not built: reuse of the splitter's D2" in raw and "merging re-evaluated on the groups' peaks" in raw
    assert _lib.ABI_VERSION == 13 and _lib.symbols("camo_split_merge.h") == ("camo_split_merge_workspace_bytes", "camo_split_merge")
    for header in ("camo_split.h", "camo_split_geo.h"):
        other = open(os.path.join(ROOT, "include", header)).read()
        assert "h-maxima" not in other and "camo_split_merge.h" in other and "per-component absolute radius" in other


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L, S = _lib.lib(), _lib.SEG_WF_MAX_SIDE
    ws = L.camo_split_merge_workspace_bytes
    assert ws(1, 1, 1) > 0 and ws(1, 1, 1) % 256 == 0 and ws(2, 45, 70) > ws(1, 45, 70) > ws(1, 45, 69) and ws(1, 3, S) > 0 and ws(1, S, S) > 0
    for bad in ((0, 8, 8), (65536, 1, 1), (1, 0, 8), (1, 8, -1), (1, S + 1, 8), (1, 8, S + 1), (257, S, S), (-1, 8, 8)):
        assert ws(*bad) == 0, bad
    p, q, r, big = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), ctypes.c_void_p(0x600000), 1 << 40
    good = dict(labels=p, parts=r, pred=None, stride=0, N=2, H=8, W=8, num=4, den=5, rows=64, out=q, table=ctypes.c_void_p(0x300000),
                counts=ctypes.c_void_p(0x400000), ws=ctypes.c_void_p(0x500000), nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return L.camo_split_merge(a["labels"], a["parts"], a["pred"], a["stride"], a["N"], a["H"], a["W"], a["num"], a["den"], a["rows"], a["out"], a["table"],
                                  a["counts"], a["ws"], a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=S + 1), dict(W=S + 1), dict(num=0), dict(num=6), dict(den=17, num=17), dict(den=0, num=0),
               dict(num=-4, den=-5), dict(rows=0), dict(rows=_lib.INST_MAX_ROWS), dict(pred=p, stride=63), dict(pred=p, stride=-1), dict(labels=None),
               dict(parts=None), dict(out=None), dict(table=None), dict(counts=None), dict(ws=None), dict(out=p), dict(out=r),
               dict(out=ctypes.c_void_p(0x100000 + 2 * 8 * 8 * 4 - 4)), dict(parts=ctypes.c_void_p(0x200000 + 4)), dict(table=ctypes.c_void_p(0x300004)),
               dict(ws=ctypes.c_void_p(0x500080)), dict(nbytes=ws(2, 8, 8) - 1), dict(nbytes=0)):
        assert call(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def _run(name, **kw):
    lab, parts, merge, rows = case(name)
    return run(lab, parts, merge=merge, rows=rows, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_merge_equals_the_restatement_bytewise(name):
    same_bytes(_run(name), want(name), name, NAMES)


@pytest.mark.gpu
def test_merge_on_workspace_of_every_fill_and_after_a_larger_call():
    for fill, ws_fill in ((0x00, 0x00), (0xFF, 0x7F), (0x7F, 0xA5)):
        same_bytes(_run("bad_part", fill=fill, ws_fill=ws_fill), want("bad_part"), (fill, ws_fill), NAMES)
    # The workspace is a function of N, H and W alone, and so are the outputs: the larger call is one of the same sizes that leaves
    # more behind -- 786 part ids in the place of 3, up to 1014, with passes and links of their own, other contents in every array.
    lab, parts, merge, rows = case("chain_3_5")
    every = (np.arange(lab.size, dtype=np.int32).reshape(lab.shape) % 1024 + 1) * (lab[:, ::-1] > 0)
    larger = merge_call(np.ascontiguousarray(lab[:, ::-1]), every, merge=(1, 16), rows=rows)
    assert larger.ws == merge_call(lab, parts).ws and len(np.unique(every)) == 787 and every.max() == 1014
    same_bytes(_run("chain_3_5", before=(larger,)), want("chain_3_5"), "after a larger call", NAMES)


@pytest.mark.gpu
def test_sq_with_and_without_pred_and_a_channel_in_place():
    lab, parts, merge, rows = case("bad_part")
    pred = _pred(lab.shape, 3)
    pred[0, 0, :3] = (np.nan, -2.0, 7.0)
    ref = M.merge(lab, parts, pred, merge, rows)
    got = run(lab, parts, pred, merge=merge, rows=rows)
    same_bytes(got, ref, "with pred", NAMES)
    assert (got["table"][[0, 2], :, 7] > 0).any() and not got["table"][1].any() and not want("bad_part")["table"][..., 7].any()
    maps = _pred((3, 3) + lab.shape[1:], 5)
    ref = M.merge(lab, parts, maps[:, 1], merge, rows)
    same_bytes(run(lab, parts, maps, 1, merge=merge, rows=rows), ref, "channel 1", NAMES)
    assert ref["table"].tobytes() != M.merge(lab, parts, maps[:, 0], merge, rows)["table"].tobytes()


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_agree():
    names = ("neck_31", "neck_29")
    lab = np.concatenate([case(n)[0] for n in names] + [case("neck_31")[0][:, ::-1]])
    parts = np.concatenate([case(n)[1] for n in names] + [case("neck_31")[1][:, ::-1]])
    pred = _pred(lab.shape, 11)
    whole = run(lab, parts, pred)
    same_bytes(run(lab, parts, pred, fill=0x00, ws_fill=0x00), whole, "two calls", NAMES)
    for n in range(3):
        one = run(lab[n:n + 1], parts[n:n + 1], pred[n:n + 1])
        same_bytes({k: v[0] for k, v in one.items()}, {k: v[n] for k, v in whole.items()}, n, NAMES)
    same_bytes(whole, M.merge(lab, parts, pred), "the batch", NAMES)
    assert whole["counts"][:, 0].tolist() == [1, 2, 1]


@pytest.mark.gpu
def test_python_surface_on_the_device():
    from camouflage_multimodal_amd import split as S
    lab, parts, merge, rows = case("lobe_euclid_4_5")
    t, p = torch.from_numpy(np.array(lab)).cuda(), torch.from_numpy(np.array(parts)).cuda()
    out = S.merge_parts(t, p, None, merge, rows)
    same_bytes({k: v.cpu().numpy() for k, v in out.items()}, want("lobe_euclid_4_5"), "merge_parts", NAMES)
    one = S.merge_parts(t[0], p[0])
    assert tuple(one["labels"].shape) == (1, 64, 120) and torch.equal(one["labels"], out["labels"])
    pred = torch.from_numpy(_pred((1, 3, 64, 120), 2)).cuda()
    ref = M.merge(lab, parts, pred[:, 2].cpu().numpy(), merge, rows)
    same_bytes({k: v.cpu().numpy() for k, v in S.merge_parts(t, p, pred[:, 2]).items()}, ref, "a channel view", NAMES)
    with pytest.raises(Exception, match="parts is on cpu"):
        S.merge_parts(t, p.cpu())
