"""Geodesic growth for the instance splitter (include/camo_split_geo.h): camo_split_instances_geodesic and
camo_split_geodesic_resume against tests/split_geo_ref.py, byte for byte.

CPU: the heap Dijkstra of the restatement against Bellman-Ford sweeps to a fixed point on maps of at most 16 x 16; for every input of
the GPU tests a check, on the references alone, that the input has the property it is named for; the header against the binding; the
source's launch lists; the library's argument checks with pointers that are never dereferenced; ``split_options`` with the new keys.
GPU: every buffer of every call sits between guards on memory the call did not clear (tests/guarded.py, tests/raw_calls.py), and the
device's parts are checked for being connected by a flood fill that knows nothing of the restatement.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import split_geo_ref as G
import split_ref as R
from conftest import ROOT
from instances_ref import components
from raw_calls import Call, execute, same_bytes
from test_split import case as euclid_case

NAMES = ("labels", "table", "counts")
DEFAULT = dict(ratio=(7, 10), min_core=0, max_split=4, rows=64)
TILE = 32
AMPLE = 64                                                     # rounds: more than any input here needs (the CPU tests say how many tiles each crosses)


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def _disc(lab, cy, cx, r, value):
    yy, xx = np.mgrid[:lab.shape[0], :lab.shape[1]]
    lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = value


def _polyline(points):
    """The pixels of a path through ``points``: every leg horizontal, vertical or at 45 degrees, in order, none twice."""
    path = [tuple(points[0])]
    for (y1, x1) in points[1:]:
        y0, x0 = path[-1]
        dy, dx = np.sign(y1 - y0), np.sign(x1 - x0)
        assert dy == 0 or dx == 0 or abs(y1 - y0) == abs(x1 - x0)
        while (y0, x0) != (y1, x1):
            y0, x0 = y0 + dy, x0 + dx
            path.append((int(y0), int(x0)))
    assert len(set(path)) == len(path)
    return path


SPIRAL_POINTS = ((20, 20), (20, 25), (15, 25), (15, 15), (25, 15), (25, 30), (10, 30), (10, 10), (30, 10), (30, 35), (5, 35), (5, 5), (36, 5))
# from the disc on the tile border x = 31 | 32 to the disc at (5, 20): 8 tile borders, one of them the corner (63 | 64, 63 | 64)
SERPENT_POINTS = ((16, 32), (16, 90), (40, 90), (40, 87), (87, 40), (87, 10), (50, 10), (50, 45), (28, 45), (28, 5), (5, 5), (5, 20))


def tile_crossings(path):
    return sum((a[0] // TILE, a[1] // TILE) != (b[0] // TILE, b[1] // TILE) for a, b in zip(path, path[1:]))


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (labels int32 [N, H, W], parameters of the call).  Read-only: the arrays are shared."""
    p = dict(DEFAULT)
    if name == "spiral":                                      # two turns, a corridor 2 pixels wide, a blob at the centre and one at the outer end
        lab = np.zeros((1, 41, 41), np.int32)
        for y, x in _polyline(SPIRAL_POINTS):
            lab[0, y:y + 2, x:x + 2] = 1
        _disc(lab[0], 20, 20, 3, 1)
        _disc(lab[0], 36, 5, 3, 1)
    elif name == "serpentine":                                # a corridor 1 pixel wide over 3 x 3 tiles
        lab = np.zeros((1, 96, 96), np.int32)
        for y, x in _polyline(SERPENT_POINTS):
            lab[0, y, x] = 1
        _disc(lab[0], 16, 32, 3, 1)
        _disc(lab[0], 5, 20, 3, 1)
    elif name == "one_tile":                                  # 32 x 32: both cores near one end of a corridor of more pixels than a tile relaxes in two launches
        lab = np.zeros((1, 32, 32), np.int32)
        pts = [(3, 4)]
        for i, y in enumerate(range(3, 30, 2)):
            pts += [(y, 27 if i % 2 == 0 else 4)] + ([(y + 2, 27 if i % 2 == 0 else 4)] if y < 29 else [])
        for y, x in _polyline(pts):
            lab[0, y, x] = 1
        lab[0, 1:4, 1:4] = 1
        lab[0, 0:3, 12:15] = 1
    elif name == "tie":                                       # a symmetric dumbbell: column 20 is as far from one core as from the other
        lab = np.zeros((1, 17, 41), np.int32)
        _disc(lab[0], 8, 8, 6, 1)
        _disc(lab[0], 8, 32, 6, 1)
        lab[0, 7:10, 8:33] = 1
    elif name == "touching":                                  # ids 1 and 2 share a border of 25 columns; a tooth of id 2 sends id 1's bar on a detour
        lab = np.zeros((1, 30, 49), np.int32)
        for x0 in (2, 36):
            lab[0, 4:15, x0:x0 + 11] = 1
            lab[0, 15:26, x0:x0 + 11] = 2
        lab[0, 12:15, 12:37] = 1
        lab[0, 15:18, 12:37] = 2
        lab[0, 12:15, 17:20] = 2
        lab[0, 9:12, 15:22] = 1
        p["min_core"] = 2                                     # (the tooth's tip is a core of one pixel: dropped, an ordinary pixel of id 2)
    elif name == "fragment":                                  # a dumbbell and, 2 pixels off its right disc, a speck of the same id
        lab = np.zeros((1, 17, 48), np.int32)
        _disc(lab[0], 8, 8, 6, 1)
        _disc(lab[0], 8, 32, 6, 1)
        lab[0, 7:10, 8:33] = 1
        lab[0, 7:10, 41:45] = 1
    elif name in ("slot_limit", "truncation", "core_drop_above", "core_drop_at", "seams", "two_discs_low_ratio", "two_discs"):
        lab, p = euclid_case(name)                            # tests/test_split.py's inputs, whose properties its CPU tests hold
    elif name in ("1x40", "40x1"):                            # id 1 in two runs that do not touch (two cores, neither reaches the other run), id 2 whole
        row = np.zeros(40, np.int32)
        row[1:10], row[5], row[12:30] = 1, 0, 2
        lab = row.reshape((1, 1, 40) if name == "1x40" else (1, 40, 1))
    elif name == "3x7":
        lab, p["ratio"] = np.ones((1, 3, 7), np.int32), (1, 2)
        lab[0, 0, 2:5] = lab[0, 2, 2:5] = 0
    elif name.startswith("blobs"):                            # seeded discs of one component each, joined by thick and thin bridges
        _, H, W, seed = name.split("_")
        H, W, rs = int(H), int(W), np.random.RandomState(int(seed))
        mask = np.zeros((H, W), bool)
        centres = [(rs.randint(4, H - 4), rs.randint(4, W - 4), rs.randint(3, 7)) for _ in range(6)]
        for cy, cx, r in centres:
            yy, xx = np.mgrid[:H, :W]
            mask |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        for (ay, ax, _), (by, bx, _) in zip(centres, centres[1:]):
            for y, x in _polyline([(ay, ax), (ay, bx), (by, bx)]):
                mask[y, x] = True
        mask[0, :], mask[-1, :], mask[:, 0], mask[:, -1] = False, False, False, False
        lab, n = components(mask, 8)
        lab, p["ratio"] = lab[None], (1, 2)
    elif name == "batch":                                     # N = 3: an image that is split, an empty one, one with no background
        lab = np.zeros((3, 40, 64), np.int32)
        lab[0] = euclid_case("two_discs")[0][0]
        lab[2, :, :32], lab[2, :, 32:] = 1, 2
    else:
        raise KeyError(name)
    lab = np.ascontiguousarray(lab, np.int32)
    lab.setflags(write=False)
    return lab, p


CONNECTED = ["spiral", "serpentine", "one_tile", "tie", "touching", "3x7", "blobs_33_65_1", "blobs_64_96_2", "blobs_96_96_3", "blobs_45_70_4", "slot_limit",
             "truncation", "core_drop_above", "core_drop_at", "seams", "two_discs", "batch"]       # every id is 8-connected: so must every part be
CASES = CONNECTED + ["fragment", "1x40", "40x1", "two_discs_low_ratio"]


@functools.lru_cache(maxsize=None)
def want(name):
    lab, p = case(name)
    return G.split(lab, None, p["ratio"], p["min_core"], p["max_split"], p["rows"])


@functools.lru_cache(maxsize=None)
def euclid(name):
    lab, p = case(name)
    return R.split(lab, None, p["ratio"], p["min_core"], p["max_split"], p["rows"])


def pieces(out, k):
    return components(out == k, 8)[1]


def parts_are_connected_and_hold_their_cores(out, lab, ratio, min_core, max_split, what):
    """On ONE output map, by flood fill: every part of a split id is one 8-connected piece and contains its core.  The cores and the
    numbering come from split_ref's flood fill and the header's step 5, not from the growth."""
    ids = R.read_ids(lab)
    number, core_ids, areas, _ = R.cores(ids, R.distance2(ids), *ratio)
    kept = [c for c in range(1, len(core_ids) + 1) if areas[c - 1] >= min_core]
    by_id = {}
    for c in kept:
        by_id.setdefault(core_ids[c - 1], []).append(c)
    split = sorted(i for i, cs in by_id.items() if len(cs) >= 2)[:max_split]
    checked = 0
    for i in split:
        news = np.unique(out[ids == i])
        assert len(news) == len(by_id[i]), (what, i, news.tolist())
        for c, k in zip(by_id[i], news):                      # (ascending core number = ascending new id)
            assert (out[number == c] == k).all(), (what, "the core is not in its part", i, k)
            assert pieces(out, k) == 1, (what, "a part in pieces", i, k, pieces(out, k))
            checked += 1
    return checked


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------

def brute(lab, ratio=(7, 10), min_core=0, max_split=4):
    """out_labels of one small map with the growth as Bellman-Ford: every pixel's key (cost << 32 | new id) is lowered to the smallest
    of its 8 neighbours' keys of the same id plus the link, whole-image sweeps, until a sweep changes nothing."""
    ids = R.read_ids(lab)
    H, W = ids.shape
    number, core_ids, areas, _ = R.cores(ids, R.distance2(ids), *ratio)
    kept = [c for c in range(1, len(core_ids) + 1) if areas[c - 1] >= min_core]
    split = sorted({i for i in core_ids if sum(core_ids[c - 1] == i for c in kept) >= 2})[:max_split]
    out, nxt, FAR = np.zeros((H, W), np.int32), 0, np.int64(1) << 62
    for i in sorted(set(ids[ids > 0].tolist())):
        mine = ids == i
        if i not in split:
            nxt += 1
            out[mine] = nxt
            continue
        cs = [c for c in kept if core_ids[c - 1] == i]
        key = np.full((H + 2, W + 2), FAR, np.int64)
        inner = key[1:-1, 1:-1]
        for k, c in enumerate(cs):
            inner[number == c] = nxt + k + 1
        while True:
            before = key.copy()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dy or dx:
                        cand = before[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] + (np.int64(5 if dy == 0 or dx == 0 else 7) << 32)
                        np.minimum(inner, np.where(mine & (before[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] < FAR), cand, FAR), out=inner)
            inner[~mine] = FAR
            if np.array_equal(key, before):
                break
        out[mine] = np.where(inner[mine] < FAR, inner[mine] & 0xFFFFFFFF, nxt + 1)
        nxt += len(cs)
    return out


def test_the_restatement_is_the_fixed_point_of_bellman_ford():
    maps = [case("3x7")]
    bars = np.zeros((1, 16, 16), np.int32)                    # two squares and a one-pixel bar; a second id of the same shape below, touching
    bars[0, 1:6, 1:6], bars[0, 1:6, 10:15], bars[0, 3, 6:10] = 1, 1, 1
    bars[0, 6:11, 1:6], bars[0, 6:11, 10:15], bars[0, 8, 6:10] = 2, 2, 2
    maps.append((bars, dict(DEFAULT)))
    hook = np.zeros((1, 16, 16), np.int32)                    # a U: the Euclidean and the geodesic cut differ
    hook[0, 1:15, 1:4], hook[0, 12:15, 1:15], hook[0, 1:15, 12:15], hook[0, 1:6, 1:7], hook[0, 1:5, 9:15] = 1, 1, 1, 1, 1
    maps.append((hook, dict(DEFAULT, ratio=(1, 2))))
    for seed in range(12):
        mask = np.random.RandomState(seed).rand(16, 16) < 0.62
        maps.append((components(mask, 8)[0][None].astype(np.int32), dict(DEFAULT, ratio=(1, 2))))
    split = 0
    for lab, p in maps:
        got, _, counts, _ = G.split_image(lab[0], None, p["ratio"], p["min_core"], p["max_split"], p["rows"])
        assert np.array_equal(got, brute(lab[0], p["ratio"], p["min_core"], p["max_split"]))
        assert counts.tolist() == R.split_image(lab[0], None, p["ratio"], p["min_core"], p["max_split"], p["rows"])[2].tolist()
        split += int(counts[1])
    assert split >= 8                                          # the comparison is not one of maps that nothing happens on


def test_case_spiral():
    """What the fixture is for, on the references: the Euclidean parts come in pieces, the geodesic ones do not, and the two differ."""
    lab, p = case("spiral")
    e, g = euclid("spiral")["labels"][0], want("spiral")["labels"][0]
    assert components(lab[0] > 0, 8)[1] == 1 and want("spiral")["counts"].tolist() == euclid("spiral")["counts"].tolist() == [[2, 1, 0, 0]]
    assert max(pieces(e, 1), pieces(e, 2)) >= 2 and pieces(g, 1) == pieces(g, 2) == 1 and int((e != g).sum()) > 0
    assert parts_are_connected_and_hold_their_cores(g, lab[0], p["ratio"], 0, 4, "spiral") == 2
    with pytest.raises(AssertionError, match="a part in pieces"):
        parts_are_connected_and_hold_their_cores(e, lab[0], p["ratio"], 0, 4, "the Euclidean cells")          # (the flood-fill check itself)


def test_case_serpentine_and_one_tile():
    lab, _ = case("serpentine")
    path = _polyline(SERPENT_POINTS)
    assert tile_crossings(path) == 8 and want("serpentine")["counts"].tolist() == [[2, 1, 0, 0]]
    assert (63, 64) in path and (64, 63) in path and lab[0, 63, 63] == 0 and lab[0, 64, 64] == 0      # joined by a diagonal link across a tile corner only
    core = want("serpentine")["info"][0]["core"]
    assert core[16, 31] > 0 and core[16, 31] == core[16, 32]                                          # one core in two tiles
    run, longest = 1, 1                                                                               # every stretch inside one tile relaxes in one launch
    for a, b in zip(path, path[1:]):
        run = run + 1 if (a[0] // TILE, a[1] // TILE) == (b[0] // TILE, b[1] // TILE) else 1
        longest = max(longest, run)
    assert longest + 8 < 4 * TILE
    out = want("serpentine")["labels"][0]
    assert out[16, 60] == 2 and out[28, 20] == 1 and pieces(out, 1) == pieces(out, 2) == 1
    lab, _ = case("one_tile")
    w = want("one_tile")
    assert w["counts"].tolist() == [[2, 1, 0, 0]] and components(lab[0] > 0, 8)[1] == 1
    assert w["info"][0]["cost"].max() > 5 * 4 * TILE * 2                                              # farther from both cores than two launches' sweeps reach


def test_case_tie_touching_fragment():
    lab, p = case("tie")
    w = want("tie")
    info = w["info"][0]
    (c1, k1), (c2, k2) = sorted(info["new_of"].items())
    one = G.grow(lab[0] == 1, {(int(y), int(x)): k1 for y, x in np.argwhere(info["core"] == c1)})
    two = G.grow(lab[0] == 1, {(int(y), int(x)): k2 for y, x in np.argwhere(info["core"] == c2)})
    ties = [q for q in one if one[q][0] == two[q][0]]
    assert len(ties) >= 3 and all(x == 20 for _, x in ties) and all(w["labels"][0][q] == 1 for q in ties) and k1 == 1
    lab, p = case("touching")
    w = want("touching")
    assert w["counts"].tolist() == [[4, 2, 1, 0]] and int(((lab[0, :-1] == 1) & (lab[0, 1:] == 2)).sum()) >= 25
    info = w["info"][0]
    seeds = {(int(y), int(x)): info["new_of"][int(info["core"][y, x])] for y, x in np.argwhere(np.isin(info["core"], [c for c in info["kept"] if info["core_ids"][c - 1] == 1]))}
    crossing = G.grow(lab[0] > 0, seeds)                       # id 1's cores let loose over both ids: a shorter way under the tooth
    assert any(crossing[q][1] != w["labels"][0][q] for q in map(tuple, np.argwhere(lab[0] == 1)))
    assert set(np.unique(w["labels"][0][lab[0] == 1])) == {1, 2} and set(np.unique(w["labels"][0][lab[0] == 2])) == {3, 4}
    lab, p = case("fragment")
    w = want("fragment")
    assert components(lab[0] > 0, 8)[1] == 2 and w["counts"].tolist() == [[2, 1, 0, 0]]
    assert (w["labels"][0, 7:10, 41:45] == 1).all() and (w["info"][0]["cost"][7:10, 41:45] == -1).all()
    assert (euclid("fragment")["labels"][0, 7:10, 41:45] == 2).all()                                  # (nearer to the second core as the crow flies)


def test_case_the_rest():
    assert want("slot_limit")["counts"].tolist() == [[5, 2, 0, 1]] and want("truncation")["counts"].tolist() == [[6, 3, 0, 0]]
    assert want("core_drop_above")["counts"].tolist() == [[1, 0, 1, 0]] and want("core_drop_at")["counts"].tolist() == [[2, 1, 0, 0]]
    assert want("two_discs_low_ratio")["counts"].tolist() == [[1, 0, 0, 0]]
    same_bytes(want("two_discs_low_ratio"), euclid("two_discs_low_ratio"), "nothing qualifies", NAMES)
    for name in ("1x40", "40x1"):
        assert want(name)["counts"].tolist() == [[3, 1, 0, 0]] and want(name)["labels"].reshape(-1)[[1, 4, 6, 9, 12]].tolist() == [1, 1, 2, 2, 3]
    assert want("3x7")["labels"][0].tolist() == [[1, 1, 0, 0, 0, 2, 2], [1, 1, 1, 1, 2, 2, 2], [1, 1, 0, 0, 0, 2, 2]]
    assert sorted(case(n)[0].shape[1:] for n in ("blobs_33_65_1", "1x40", "40x1", "3x7")) == [(1, 40), (3, 7), (33, 65), (40, 1)]
    for name in ("blobs_33_65_1", "blobs_64_96_2", "blobs_96_96_3", "blobs_45_70_4"):
        assert want(name)["counts"][0, 1] >= 1, name
    assert want("batch")["counts"].tolist() == [[2, 1, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0]] and (case("batch")[0][2] > 0).all()
    for name in CONNECTED:
        lab, p = case(name)
        for n in range(lab.shape[0]):
            assert components(lab[n] > 0, 8)[1] == len(np.unique(lab[n][lab[n] > 0])) or name in ("seams", "batch", "touching"), name
            parts_are_connected_and_hold_their_cores(want(name)["labels"][n], lab[n], p["ratio"], p["min_core"], p["max_split"], name)


# ---- CPU: the header, the source, the library's checks, the options -----------------------------------------------------------------

def test_header_constants_symbols_and_launch_lists():
    from camouflage_multimodal_amd import _lib
    raw = open(os.path.join(ROOT, "include", "camo_split_geo.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    assert int(m["CAMO_SPLIT_GEO_TILE"]) == _lib.SPLIT_GEO_TILE == TILE and int(m["CAMO_SPLIT_GEO_MAX_ROUNDS"]) == _lib.SPLIT_GEO_MAX_ROUNDS >= AMPLE
    assert int(m["CAMO_SPLIT_GEO_LAUNCHES"]) == _lib.SPLIT_GEO_LAUNCHES and int(m["CAMO_SPLIT_GEO_RESUME_LAUNCHES"]) == _lib.SPLIT_GEO_RESUME_LAUNCHES
    assert _lib.symbols("camo_split_geo.h") == ("camo_split_geodesic_workspace_bytes", "camo_split_instances_geodesic", "camo_split_geodesic_resume")
    assert "PARITY UNPINNED" in raw and _lib.ABI_VERSION == 13
    old = open(os.path.join(ROOT, "include", "camo_split.h")).read()
    assert "Not built" in old and "geodesic" not in old.split("Not built")[1].split("\n\n")[0] and "RegionGraphFineTuner" not in old
    src = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "split_geo.hip")).read()
    inl = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "split_inl.h")).read()
    for s in (src, inl):
        assert "hipMalloc" not in s and "Synchronize" not in s and not re.search(r"atomic(Add|Min|Max|CAS|Exch)\s*\(\s*\(?\s*(float|double)", s)
    assert "cooperative" not in src.lower() and "grid" not in re.sub(r"//[^\n]*", "", src).replace("gridDim", "") and not re.search(r"\bwhile\b", src.split("namespace {")[1])
    # the resume: one launch inside the one loop over the rounds, two after it; the first call: eleven launches, then the resume's
    resume = src.split("int launch_split_geo_resume(")[1].split("\n}\n")[0].split("{", 1)[1]
    loop, rest = resume.split("for (int r = 0; r < rounds; ++r)")
    assert "hipLaunchKernelGGL(" not in loop and rest.count("hipLaunchKernelGGL(") == 1 + _lib.SPLIT_GEO_RESUME_LAUNCHES
    assert rest.lstrip().startswith("hipLaunchKernelGGL(split_geo_grow_kernel") and not re.search(r"\b(for|while|if)\b", rest)
    first = src.split("int launch_split_geo(")[1].split("{", 1)[1]
    assert first.count("hipLaunchKernelGGL(") + _lib.SPLIT_GEO_RESUME_LAUNCHES == _lib.SPLIT_GEO_LAUNCHES and not re.search(r"\b(for|while|if)\b", first)
    assert first.count("launch_split_geo_resume(") == 1
    euclid_launcher = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "split.hip")).read().split("int launch_split(")[1]
    common = re.findall(r"hipLaunchKernelGGL\((\w+)", euclid_launcher)[:10]
    assert common[-1] == "split_rank_kernel" and re.findall(r"hipLaunchKernelGGL\((\w+)", first)[:10] == common


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L, S = _lib.lib(), _lib.SEG_WF_MAX_SIDE
    ws = L.camo_split_geodesic_workspace_bytes
    assert ws(1, 1, 1, 1) > 0 and ws(1, 1, 1, 1) % 256 == 0 and ws(2, 45, 70, 4) > ws(1, 45, 70, 4) and ws(1, S, S, 8) > 0
    assert ws(2, 512, 512, 8) < L.camo_split_workspace_bytes(2, 512, 512, 8)                  # no site planes: 8 bytes a pixel for 16
    for bad in ((0, 8, 8, 4), (65536, 1, 1, 4), (1, 0, 8, 4), (1, 8, -1, 4), (1, S + 1, 8, 4), (1, 8, S + 1, 4), (257, S, S, 4), (1, 8, 8, 0), (1, 8, 8, 9)):
        assert ws(*bad) == 0, bad
    p, q, big = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), 1 << 40
    good = dict(labels=p, pred=None, stride=0, N=2, H=8, W=8, num=7, den=10, min_core=0, max_split=4, rows=64, out=q, table=ctypes.c_void_p(0x300000),
                counts=ctypes.c_void_p(0x400000), ws=ctypes.c_void_p(0x500000), nbytes=big, rounds=4, pending=ctypes.c_void_p(0x600000))
    for fn in (L.camo_split_instances_geodesic, L.camo_split_geodesic_resume):
        def call(**kw):
            a = dict(good, **kw)
            return fn(a["labels"], a["pred"], a["stride"], a["N"], a["H"], a["W"], a["num"], a["den"], a["min_core"], a["max_split"], a["rows"], a["out"],
                      a["table"], a["counts"], a["ws"], a["nbytes"], None, a["rounds"], a["pending"])
        for kw in (dict(rounds=0), dict(rounds=-1), dict(rounds=_lib.SPLIT_GEO_MAX_ROUNDS + 1), dict(pending=None), dict(N=0), dict(N=65536), dict(H=0),
                   dict(W=-3), dict(H=S + 1), dict(W=S + 1), dict(num=0), dict(num=10), dict(den=17), dict(den=1, num=1), dict(min_core=-1), dict(max_split=0),
                   dict(max_split=9), dict(rows=0), dict(rows=_lib.INST_MAX_ROWS), dict(pred=p, stride=63), dict(labels=None), dict(out=None), dict(table=None),
                   dict(counts=None), dict(ws=None), dict(out=p), dict(out=ctypes.c_void_p(0x100000 + 2 * 8 * 8 * 4 - 4)),
                   dict(labels=ctypes.c_void_p(0x200000 + 4)), dict(table=ctypes.c_void_p(0x300004)), dict(ws=ctypes.c_void_p(0x500080)),
                   dict(nbytes=ws(2, 8, 8, 4) - 1), dict(nbytes=0)):
            assert call(**kw) == -1, kw                                  # CAMO_E_ARG
            assert L.camo_last_error()


def test_split_options_with_growth():
    from camouflage_multimodal_amd import split as S
    four = {"ratio": (7, 10), "min_core": 0, "max_split": 4, "max_instances": 64}
    assert S.split_options(True) == four and S.split_options({}) == four and S.split_options(None) is None and S.split_options(False) is None
    assert S.split_options({"ratio": [1, 2], "max_split": 8}) == {"ratio": (1, 2), "min_core": 0, "max_split": 8, "max_instances": 64}
    assert S.split_options({"min_core": 3, "max_instances": 7}) == dict(four, min_core=3, max_instances=7)
    assert S.split_options({"growth": "geodesic"}) == dict(four, growth="geodesic")
    assert S.split_options({"growth": "geodesic", "rounds": 5, "max_split": 2}) == dict(four, growth="geodesic", rounds=5, max_split=2)
    assert S.split_options({"growth": "euclidean"}) == dict(four, growth="euclidean")
    for bad, word in (({"growth": "watershed"}, "growth"), ({"growth": None}, "growth"), ({"growth": "geodesic", "rounds": 0}, "rounds"),
                      ({"growth": "geodesic", "rounds": 1.5}, "rounds"), ({"growth": "geodesic", "rounds": True}, "rounds"),
                      ({"growth": "geodesic", "rounds": 1025}, "rounds"), ({"rounds": 4}, "rounds"), ({"radius": 3}, "split must be"),
                      ({"growth": "geodesic", "radius": 3}, "split must be")):
        with pytest.raises(ValueError, match="^" + word):
            S.split_options(bad)
    lab = torch.zeros(1, 8, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="^growth"):
        S.split_instances(lab, growth="geo")
    with pytest.raises(ValueError, match="^rounds"):
        S.split_instances(lab, growth="geodesic", rounds=0)
    from camouflage_multimodal_amd import _lib
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        S.split_instances(lab, growth="geodesic")


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def geo_call(lab, pred=None, channel=0, ratio=(7, 10), min_core=0, max_split=4, rows=64, rounds=AMPLE, resumes=()):
    """camo_split_instances_geodesic with ``rounds``, then one camo_split_geodesic_resume per entry of ``resumes`` (its rounds) on the
    same buffers, as ONE raw_calls.Call: the harness fills the workspace before a Call, and a resume needs what the call left."""
    from camouflage_multimodal_amd import _lib
    L, (N, H, W) = _lib.lib(), lab.shape
    at, stride, ins = 0, 0, {"labels": np.asarray(lab, np.int32)}
    if pred is not None:
        ins["pred"] = pred = np.asarray(pred, np.float32)
        at, stride = (4 * channel * H * W, pred.shape[1] * H * W) if pred.ndim == 4 else (0, H * W)
    nbytes = L.camo_split_geodesic_workspace_bytes(N, H, W, max_split)
    assert nbytes > 0 and nbytes % 256 == 0
    outs = {"labels_out": ((N, H, W), np.int32), "table": ((N, rows, 8), np.int64), "counts": ((N, 4), np.int32), "pending": ((N,), np.int32)}

    def invoke(p, w, nb):
        args = (p["labels"], p["pred"] + at if pred is not None else None, stride, N, H, W, ratio[0], ratio[1], min_core, max_split, rows, p["labels_out"],
                p["table"], p["counts"], w, nb, torch.cuda.current_stream().cuda_stream)
        rc = L.camo_split_instances_geodesic(*args, rounds, p["pending"])
        for r in resumes:
            rc = rc or L.camo_split_geodesic_resume(*args, r, p["pending"])
        return rc
    return Call(outs, nbytes, invoke, ins)


def _run(lab, pred=None, channel=0, fill=0xA5, ws_fill=0xFF, **p):
    got = execute(geo_call(lab, pred, channel, **p), fill, ws_fill=ws_fill, skew=8)
    return {"labels": got["labels_out"], "table": got["table"], "counts": got["counts"], "pending": got["pending"]}


def _pred(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_geodesic_split_equals_the_restatement_bytewise(name):
    lab, p = case(name)
    got = _run(lab, **p)
    assert not got["pending"].any(), got["pending"].tolist()
    same_bytes(got, want(name), name, NAMES)
    if name in CONNECTED:                                      # on the device's own bytes, by flood fill
        for n in range(lab.shape[0]):
            parts_are_connected_and_hold_their_cores(got["labels"][n], lab[n], p["ratio"], p["min_core"], p["max_split"], name)


@pytest.mark.gpu
def test_rounds_pending_and_resume_on_the_serpentine():
    lab, p = case("serpentine")
    crossings = tile_crossings(_polyline(SERPENT_POINTS))
    first = _run(lab, rounds=1, **p)
    assert first["pending"][0] > 0                             # the cores' tiles ran; the tile the corridor enters next is flagged
    same_bytes(first, want("serpentine"), "counts do not wait for the growth", ("counts",))
    assert np.array_equal(first["labels"] > 0, lab > 0) and set(np.unique(first["labels"])) == {0, 1, 2}
    needed = None
    for resumes in range(1, crossings + 2):
        got = _run(lab, rounds=1, resumes=(1,) * resumes, **p)
        if not got["pending"].any():
            needed = resumes
            break
    assert needed is not None and needed <= crossings + 1, "more resumes of one round than the corridor crosses tile borders, plus one"
    same_bytes(got, want("serpentine"), "resumed", NAMES)
    same_bytes(_run(lab, rounds=1, resumes=(1,) * needed + (3,), fill=0x00, ws_fill=0x00, **p), want("serpentine"), "a resume with nothing left to do", NAMES)
    same_bytes(_run(lab, rounds=2, resumes=(AMPLE,), **p), want("serpentine"), "one long resume", NAMES)


@pytest.mark.gpu
def test_a_tile_still_changing_at_its_bound_flags_itself():
    lab, p = case("one_tile")
    assert _run(lab, rounds=1, **p)["pending"].tolist() == [1] and _run(lab, rounds=2, **p)["pending"].tolist() == [1]
    got = _run(lab, rounds=1, resumes=(2, 4, 8), **p)
    assert got["pending"].tolist() == [0]
    same_bytes(got, want("one_tile"), "one tile over several rounds", NAMES)


@pytest.mark.gpu
def test_workspace_of_every_fill_pred_and_its_channel():
    lab, p = case("seams")
    for fill, ws_fill in ((0x00, 0x00), (0xFF, 0x7F), (0x7F, 0xA5)):
        same_bytes(_run(lab, fill=fill, ws_fill=ws_fill, **p), want("seams"), (fill, ws_fill), NAMES)
    maps = _pred((3, 3) + lab.shape[1:], 5)
    maps[0, 1, 0, :3] = (np.nan, -2.0, 7.0)
    ref = G.split(lab, maps[:, 1], p["ratio"], p["min_core"], p["max_split"], p["rows"])
    got = _run(lab, maps, 1, **p)
    same_bytes(got, ref, "channel 1", NAMES)
    assert (got["table"][..., 7] > 0).any() and ref["table"].tobytes() != G.split(lab, maps[:, 0], p["ratio"], p["min_core"], p["max_split"], p["rows"])["table"].tobytes()
    same_bytes(_run(lab, maps[:, 2].copy(), **p), G.split(lab, maps[:, 2], p["ratio"], p["min_core"], p["max_split"], p["rows"]), "a plane", NAMES)


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_agree():
    lab, p = case("batch")
    pred = _pred(lab.shape, 11)
    whole = _run(lab, pred, **p)
    same_bytes(_run(lab, pred, fill=0x00, ws_fill=0x00, **p), whole, "two calls", NAMES + ("pending",))
    for n in range(3):
        one = _run(lab[n:n + 1], pred[n:n + 1], **p)
        same_bytes({k: v[0] for k, v in one.items()}, {k: v[n] for k, v in whole.items()}, n, NAMES + ("pending",))
    same_bytes(whole, G.split(lab, pred), "the batch", NAMES)


@pytest.mark.gpu
def test_where_nothing_qualifies_the_output_is_the_euclidean_calls():
    from test_split import _run as euclid_run
    lab, p = case("two_discs_low_ratio")
    same_bytes(_run(lab, **p), euclid_run(lab, **p), "nothing qualifies", NAMES)
