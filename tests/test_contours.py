"""Instance contours (include/camo_contours.h, camouflage_multimodal_amd/contours.py).

CPU: the sequential restatement (tests/contours_ref.py) against statements that do not follow cracks -- its polygons rasterised by the
restatement of COCO's rleFrPoly (tests/poly_ref.py) give the ids back, the a2 give the areas, scipy counts the components --, the host
side of the Python surface on the restatement's arrays, every ``ValueError`` by name, the header's constants, and the library's
argument checks (no launch, no device).  GPU: ``camo_contours`` byte for byte against the restatement between guards
(tests/contours_calls.py) on outputs filled with 0xA5 and a workspace filled with 0xFF, on both sides of the LDS / global switch, and the
round trip through ``polygons.decode_polygons``."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import contours_ref as R
import poly_ref as P
from conftest import ROOT
from contours_calls import NAMES, contours_call, run
from raw_calls import same_bytes

LDS_CRACKS = 1 << 14
BIG = 2 ** 31 - 1


def _checker(ids=None):
    yy, xx = np.indices((8, 8))
    on = ((yy + xx) % 2 == 0).astype(np.int32)
    return on if ids is None else on * ids(yy, xx)


def _hole():
    """9 x 11: a 7 x 9 block of id 1 with a 3 x 5 hole that holds a bar of id 2; a negative value in a corner."""
    m = np.zeros((9, 11), np.int32)
    m[1:8, 1:10] = 1
    m[3:6, 3:8] = 0
    m[4, 4:7] = 2
    m[0, 0] = -7
    return m


def _serpentine():
    m = np.zeros((33, 70), np.int32)
    m[0::2] = 1
    m[1::4, 69] = 1
    m[3::4, 0] = 1
    return m


def _random(H, W, seed, ids=3):
    return np.random.RandomState(seed).randint(0, ids + 1, (H, W)).astype(np.int32)


# name -> (label map [H, W], connectivity, (cracks, rings, outer rings, vertices)): the issue's figures, None where neither it nor a count by hand states one
SHAPES = {
    "one_pixel": (np.full((1, 1), 5, np.int32), 8, (4, 1, 1, 4)),
    "row_1x7": (np.full((1, 7), 1, np.int32), 8, (None, 1, 1, 4)),
    "column_5x1": (np.full((5, 1), 1, np.int32), 4, (None, 1, 1, 4)),
    "border_6x9": (np.full((6, 9), BIG, np.int32), 8, (30, 1, 1, 4)),
    "checker_4": (_checker(), 4, (128, 32, 32, 128)),
    "checker_8": (_checker(), 8, (128, 19, 1, 128)),
    "checker_three_ids": (_checker(lambda y, x: (x + y) // 2 % 3 + 1), 8, (128, None, 8, None)),
    "hole": (_hole(), 8, (56, 3, 2, 12)),
    "hole_4": (_hole(), 4, (56, 3, 2, 12)),
    "two_ids": (np.repeat(np.array([[3, 3, 3, 9, 9, 9]], np.int32), 4, axis=0), 8, (None, 2, 2, 8)),
    "serpentine": (_serpentine(), 8, (2414, 1, 1, 68)),
    "alternating_row": ((np.arange(130, dtype=np.int32) % 2 + 1)[None], 8, (None, 130, 130, 520)),
    "alternating_column": ((np.arange(130, dtype=np.int32) % 3)[:, None].copy(), 4, None),
    "random_70": (_random(70, 70, 7), 8, None),
    "random_70_4": (_random(70, 70, 7), 4, None),
}


@functools.lru_cache(maxsize=None)
def traced(name):
    img, conn, _ = SHAPES[name]
    return R.trace_image(img, conn)


def capacities(img):
    C = min(4 * img.shape[-2] * img.shape[-1], LDS_CRACKS)
    return C, max(1, C // 4), C


@functools.lru_cache(maxsize=None)
def want(name):
    img, conn, _ = SHAPES[name]
    out = dict(zip(NAMES, R.contours(img[None], conn, *capacities(img))))
    for a in out.values():
        a.setflags(write=False)
    return out


def _structure(conn):
    return np.ones((3, 3), int) if conn == 8 else ndimage.generate_binary_structure(2, 1)


def _independent(img, conn, found):
    """The rings of one image against what the label map says without following a crack."""
    H, W = img.shape
    polys = R.polygons(found)
    ids = [int(v) for v in np.unique(img) if v > 0]
    assert sorted(polys) == ids
    for i in ids:
        own = img == i
        outer, holes = polys[i]
        xor, union = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for ring in outer + holes:
            xor ^= P.polygon_mask(ring, H, W)
        for ring in outer:
            union |= P.polygon_mask(ring, H, W)
        assert (xor == own).all(), i
        assert (union == ndimage.binary_fill_holes(own, structure=_structure(4 if conn == 8 else 8))).all(), i      # (the holes' connectivity is the other one)
        assert sum(a2 for label, _, _, a2 in found if label == i) == 2 * int(own.sum()), i
        assert len(outer) == ndimage.label(own, structure=_structure(conn))[1], i
    assert [e for _, e, _, _ in found] == sorted(e for _, e, _, _ in found)
    assert all(len(v) >= 4 and a2 != 0 for _, _, v, a2 in found)


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SHAPES)
def test_restatement_against_independent_statements(name):
    img, conn, figures = SHAPES[name]
    E, found = traced(name)
    _independent(img, conn, found)
    got = (E, len(found), sum(1 for r in found if r[3] > 0), sum(len(r[2]) for r in found))
    if figures is not None:
        assert all(f is None or f == g for f, g in zip(figures, got)), got
    assert (R.crack_sides(img) == np.array([[[R.is_crack(img, y, x, s) for s in range(4)] for x in range(img.shape[1])] for y in range(img.shape[0])])).all()


def test_the_hole_ring_starts_in_the_middle_of_an_edge():
    _, found = traced("hole")
    label, e, verts, a2 = found[1]
    assert (label, e % 4, a2) == (1, 2, -30) and (e // 4) // 11 == 2 and (e // 4) % 11 == 3      # the bottom side of pixel (2, 3): (4, 3) -> (3, 3)
    assert (4, 3) not in verts and verts == [(3, 3), (3, 6), (8, 6), (8, 3)]
    assert [r[0] for r in found] == [1, 1, 2] and [r[3] for r in found] == [126, -30, 6]
    both = traced("two_ids")[1]
    assert sorted((r[0], r[2]) for r in both) == [(3, [(0, 0), (3, 0), (3, 4), (0, 4)]), (9, [(3, 0), (6, 0), (6, 4), (3, 4)])]      # two cracks on the side between them


@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_on_seeded_random_maps(conn):
    for seed, (H, W) in enumerate(((5, 7), (12, 17), (23, 9), (31, 30), (45, 45))):
        img = _random(H, W, 100 + seed)
        _independent(img, conn, R.trace_image(img, conn)[1])


def test_saddle_rule_is_the_only_effect_of_connectivity():
    img = np.array([[1, 0], [0, 1]], np.int32)
    four, eight = R.trace_image(img, 4)[1], R.trace_image(img, 8)[1]
    assert [len(r[2]) for r in four] == [4, 4] and [r[3] for r in four] == [2, 2]
    assert len(eight) == 1 and eight[0][3] == 4 and eight[0][2] == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]
    solid = np.ones((3, 4), np.int32)
    assert R.trace_image(solid, 4) == R.trace_image(solid, 8)


def test_capacities_of_the_restatement():
    img = SHAPES["serpentine"][0][None]
    full = R.contours(img, 8, 2414, 8, 80)
    assert full[2].tolist() == [[2414, 1, 68, 2414, 1, 68]] and full[0][0, 0].tolist() == [1, 0, 0, 68, 2 * int(img.sum())]
    over = R.contours(img, 8, 2413, 8, 80)
    assert over[2].tolist() == [[2414, 0, 0, 0, 0, 0]] and not over[0].any() and not over[1].any()
    short = R.contours(img, 8, 2414, 8, 67)
    assert short[2].tolist() == [[2414, 1, 68, 2414, 1, 67]] and (short[1][0] == full[1][0, :67]).all() and short[0].tobytes() == full[0].tobytes()
    board = SHAPES["checker_8"][0][None]
    rows = R.contours(board, 8, 128, 18, 128)
    assert rows[2].tolist() == [[128, 19, 128, 128, 18, 128]] and (rows[0][0] == R.contours(board, 8, 128, 19, 128)[0][0, :18]).all()


# ---- CPU: the Python surface on the restatement's arrays -----------------------------------------------------------------------------

def test_polygons_from_contours_on_reference_arrays():
    from camouflage_multimodal_amd import contours as C
    maps = np.stack([_hole(), np.zeros((9, 11), np.int32), np.pad(_checker(), ((0, 1), (0, 3)))])
    rings, xy, counts = R.contours(maps, 8, 396, 99, 396)
    per_image = C.polygons_from_contours(rings, xy, counts)
    assert per_image == C.polygons_from_contours(torch.from_numpy(rings), torch.from_numpy(xy), torch.from_numpy(counts))
    assert per_image[1] == {} and list(per_image[0]) == [1, 2]
    assert per_image[0][1] == {"polygons": [[1, 1, 10, 1, 10, 8, 1, 8]], "holes": [[3, 3, 3, 6, 8, 6, 8, 3]], "area": 48}
    assert per_image[0][2] == {"polygons": [[4, 4, 7, 4, 7, 5, 4, 5]], "holes": [], "area": 3}
    assert len(per_image[2][1]["polygons"]) == 1 and len(per_image[2][1]["holes"]) == 18 and per_image[2][1]["area"] == 32
    for n in range(3):
        assert per_image[n] == {i: {"polygons": o, "holes": h, "area": int((maps[n] == i).sum())} for i, (o, h) in R.polygons(R.trace_image(maps[n], 8)[1]).items()}
    assert C.polygons_from_contours(rings[0], xy[0], counts[0]) == per_image[:1]
    with pytest.raises(ValueError, match=r"^image 2 holds 128 cracks and 0 were taken: call trace_contours with max_cracks >= 128$"):
        C.polygons_from_contours(*R.contours(maps, 8, 127, 99, 396))
    with pytest.raises(ValueError, match=r"^image 2 holds 19 rings and 18 were written: call trace_contours with max_rings >= 19$"):
        C.polygons_from_contours(*R.contours(maps, 8, 396, 18, 396))
    with pytest.raises(ValueError, match=r"^image 0 holds 12 vertices and 11 were written: call trace_contours with max_vertices >= 12$"):
        C.polygons_from_contours(*R.contours(maps, 8, 396, 99, 11))
    with pytest.raises(ValueError, match=r"^need rings \[N, R, 5\]"):
        C.polygons_from_contours(rings[..., :4], xy, counts)
    with pytest.raises(ValueError, match=r"^need rings \[N, R, 5\]"):
        C.polygons_from_contours(rings, xy, counts[:2])


def test_coco_annotations_on_reference_arrays(tmp_path):
    import json
    from camouflage_multimodal_amd import contours as C
    from camouflage_multimodal_amd.polygons import coco_ground_truth
    maps = [_hole(), np.zeros((9, 11), np.int32)]
    polys = C.polygons_from_contours(*R.contours(np.stack(maps), 8, 396, 99, 396))
    records = [{"instances": [{"id": 1, "area": 48, "box": (1, 1, 9, 7), "score": 0.75}, {"id": 2, "area": 3, "box": (4, 4, 6, 4), "score": 0.5}], "count": 2},
               {"instances": [], "count": 0}]
    images, anns = C.coco_annotations(["b_moth", "a_owl"], [(9, 11), (9, 11)], records, polys)
    assert images == [{"id": "b_moth", "file_name": "b_moth", "height": 9, "width": 11}, {"id": "a_owl", "file_name": "a_owl", "height": 9, "width": 11}]
    assert anns == [{"id": 1, "image_id": "b_moth", "category_id": 1, "segmentation": [[1, 1, 10, 1, 10, 8, 1, 8]], "holes": [[3, 3, 3, 6, 8, 6, 8, 3]], "area": 48,
                     "bbox": [1, 1, 9, 7], "iscrowd": 0, "score": 0.75},
                    {"id": 2, "image_id": "b_moth", "category_id": 1, "segmentation": [[4, 4, 7, 4, 7, 5, 4, 5]], "holes": [], "area": 3, "bbox": [4, 4, 3, 1],
                     "iscrowd": 0, "score": 0.5}]
    numbered, anns7 = C.coco_annotations(["b_moth", "a_owl"], [(9, 11), (9, 11)], records, polys, image_ids={"b_moth": 41, "a_owl": 40}, category_id=7)
    assert [im["id"] for im in numbered] == [41, 40] and [a["image_id"] for a in anns7] == [41, 41] and {a["category_id"] for a in anns7} == {7}
    path = tmp_path / "annotations.json"
    path.write_text(json.dumps({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "camouflaged"}]}))
    truth = coco_ground_truth(str(path), ["a_owl", "b_moth.png"])
    assert truth["segmentations"] == [[], [a["segmentation"] for a in anns]] and truth["sizes"] == [(9, 11), (9, 11)] and truth["crowd_skipped"] == 0
    for a in anns:                                                   # what a reader paints: the outer rings, holes filled
        painted = np.zeros((9, 11), bool)
        for ring in a["segmentation"]:
            painted |= P.polygon_mask(ring, 9, 11)
        assert painted.sum() == a["area"] + sum(abs(_area2(h)) // 2 for h in a["holes"])


def _area2(flat):
    c = np.asarray(flat, np.int64).reshape(-1, 2)
    n = np.roll(c, -1, axis=0)
    return int((c[:, 0] * n[:, 1] - n[:, 0] * c[:, 1]).sum())


def test_python_argument_errors_by_name():
    from camouflage_multimodal_amd import _lib, contours as C
    lab = torch.zeros(2, 8, 8, dtype=torch.int32)
    for kw, word in ((dict(connectivity=6), "connectivity"), (dict(connectivity=True), "connectivity"), (dict(connectivity="8"), "connectivity"),
                     (dict(max_cracks=0), "max_cracks"), (dict(max_cracks=2.5), "max_cracks"), (dict(max_cracks=True), "max_cracks"),
                     (dict(max_cracks=257), "max_cracks = 257 exceeds 4 H W = 256"), (dict(max_rings=0), "max_rings"), (dict(max_rings="4"), "max_rings"),
                     (dict(max_rings=_lib.CONTOUR_MAX_RINGS), "max_rings"), (dict(max_vertices=0), "max_vertices"), (dict(max_vertices=-3), "max_vertices"),
                     (dict(max_vertices=_lib.CONTOUR_MAX_VERTICES), "max_vertices")):
        with pytest.raises(ValueError, match="^" + word):
            C.trace_contours(lab, **kw)
    with pytest.raises(ValueError, match="^labels must be int32"):
        C.trace_contours(lab.long())
    with pytest.raises(ValueError, match="^labels must be a tensor"):
        C.trace_contours(lab.numpy())
    with pytest.raises(ValueError, match=r"^need labels \[N, H, W\]"):
        C.encode_instance_polygons(lab[None])
    with pytest.raises(ValueError, match="^connectivity"):
        C.encode_instance_polygons(lab, connectivity=5)
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        C.trace_contours(lab)
    with pytest.raises(_lib.CamoError, match="labels is on cpu"):
        C.encode_instance_polygons(lab[0])
    assert C.contour_options(False) is False and C.contour_options(True) is True and C.contour_options(False, instances=False) is False
    with pytest.raises(ValueError, match="^polygons must be True or False"):
        C.contour_options(1)
    with pytest.raises(ValueError, match="^polygons needs instances=True"):
        C.contour_options(True, instances=False)


def test_header_constants_and_symbols():
    from camouflage_multimodal_amd import _lib
    import camouflage_multimodal_amd as pkg
    raw = open(os.path.join(ROOT, "include", "camo_contours.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    value = lambda s: eval(s, {"__builtins__": {}})                  # an integer literal or (1 << n)
    for name in ("RING_FIELDS", "COUNTS", "MAX_CRACKS", "MAX_RINGS", "MAX_VERTICES", "LDS_CRACKS"):
        assert re.fullmatch(r"\d+|\(1 << \d+\)", m["CAMO_CONTOUR_" + name]) and value(m["CAMO_CONTOUR_" + name]) == getattr(_lib, "CONTOUR_" + name), name
    assert _lib.CONTOUR_LDS_CRACKS == LDS_CRACKS and 8 * LDS_CRACKS <= 160 * 1024 < 8 * 2 * LDS_CRACKS      # the largest power of two whose two buffers of words fit a CU's LDS
    assert _lib.ABI_VERSION == 13 and _lib.symbols("camo_contours.h") == ("camo_contours_workspace_bytes", "camo_contours")
    assert "PARITY UNPINNED" in raw and "tests/contours_ref.py" in raw and "SIX launches" in raw and "5 + 2 K" in raw
    src = open(os.path.join(ROOT, "camouflage_multimodal_amd", "csrc", "contours.hip")).read()
    assert "hipMalloc" not in src and "Synchronize" not in src and not re.search(r"atomic(Add|Min|Max|CAS)\s*\(\s*\(?\s*(float|double)", src)
    from camouflage_multimodal_amd.build import SOURCES
    assert "contours.hip" in SOURCES and not {"trace_contours", "encode_instance_polygons", "coco_annotations"} & set(pkg.__all__)


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    ws = L.camo_contours_workspace_bytes
    assert ws(1, 1, 1, 4, 1, 1) > 0 and ws(1, 1, 1, 4, 1, 1) % 256 == 0 and ws(2, 45, 70, 900, 8, 8) > ws(1, 45, 70, 900, 8, 8) > ws(1, 45, 70, 600, 8, 8)
    assert ws(1, 256, 256, 2 * LDS_CRACKS, 8, 8) > 2 * ws(1, 256, 256, LDS_CRACKS, 8, 8) - ws(1, 256, 256, 1, 8, 8)      # the global form's third pair buffer
    for bad in ((0, 8, 8, 4, 1, 1), (65536, 1, 1, 4, 1, 1), (1, 0, 8, 4, 1, 1), (1, 8, -1, 4, 1, 1), (1, 8, 8, 0, 1, 1), (1, 8, 8, 257, 1, 1), (1, 8, 8, 4, 0, 1),
                (1, 8, 8, 4, 1, 0), (1, 8, 8, -4, 1, 1), (1 << 12, 128, 128, (1 << 14) + 1, 1, 1), (2, 8, 8, 4, 1 << 23 | 1, 1), (2, 8, 8, 4, 1, 1 << 25 | 1),
                (1, 1 << 14, 1 << 13, 4, 1, 1)):
        assert ws(*bad) == 0, bad
    p = ctypes.c_void_p
    good = dict(labels=p(0x100000), N=2, H=8, W=8, conn=8, C=256, R=64, V=256, rings=p(0x200000), xy=p(0x300000), counts=p(0x400000), ws=p(0x500000), nbytes=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        return L.camo_contours(a["labels"], a["N"], a["H"], a["W"], a["conn"], a["C"], a["R"], a["V"], a["rings"], a["xy"], a["counts"], a["ws"], a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(conn=6), dict(conn=0), dict(C=0), dict(C=257), dict(C=-1), dict(R=0), dict(V=0), dict(R=-2),
               dict(N=2, R=(1 << 23) + 1), dict(N=2, V=(1 << 25) + 1), dict(N=1 << 12, H=128, W=128, C=(1 << 14) + 1), dict(labels=None), dict(rings=None),
               dict(xy=None), dict(counts=None), dict(ws=None), dict(labels=p(0x100002)), dict(counts=p(0x400001)), dict(rings=p(0x200004)), dict(xy=p(0x300004)),
               dict(ws=p(0x500080)), dict(nbytes=ws(2, 8, 8, 256, 64, 256) - 1), dict(nbytes=0)):
        assert call(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_contours_equal_the_restatement_bytewise(name):
    img, conn, _ = SHAPES[name]
    same_bytes(run(img[None], conn, *capacities(img)), want(name), name, NAMES)


@pytest.mark.gpu
def test_serpentine_at_its_capacities():
    img = SHAPES["serpentine"][0][None]
    for C, Rr, V, counts in ((2414, 1, 68, [2414, 1, 68, 2414, 1, 68]), (2413, 1, 68, [2414, 0, 0, 0, 0, 0]), (2414, 1, 67, [2414, 1, 68, 2414, 1, 67]),
                             (2414, 4, 2414, [2414, 1, 68, 2414, 1, 68])):
        got = run(img, 8, C, Rr, V)
        same_bytes(got, dict(zip(NAMES, R.contours(img, 8, C, Rr, V))), (C, Rr, V), NAMES)
        assert got["counts"][0].tolist() == counts
    board = SHAPES["checker_8"][0][None]                             # one ring row short: the 19th ring's vertices are still in xy
    got = run(board, 8, 128, 18, 128)
    same_bytes(got, dict(zip(NAMES, R.contours(board, 8, 128, 18, 128))), "R one short", NAMES)
    assert got["counts"][0].tolist() == [128, 19, 128, 128, 18, 128]


@pytest.mark.gpu
def test_both_forms_give_the_same_bytes():
    """C = CAMO_CONTOUR_LDS_CRACKS is the LDS form's last capacity and twice that the global form: 256 x 256 holds both."""
    maps = np.zeros((3, 256, 256), np.int32)
    maps[0, :33, :70] = SHAPES["serpentine"][0]
    maps[1, 100:170, 3:73] = SHAPES["random_70"][0]
    maps[1, 200:208, 248:256] = SHAPES["checker_8"][0] * 5
    maps[2, 9:18, 240:251] = _hole()
    V, Rr = 8192, 2048
    lds = run(maps, 8, LDS_CRACKS, Rr, V)
    glob = run(maps, 8, 2 * LDS_CRACKS, Rr, V)
    same_bytes(lds, glob, "LDS form against global form", NAMES)
    same_bytes(lds, dict(zip(NAMES, R.contours(maps, 8, LDS_CRACKS, Rr, V))), "both against the restatement", NAMES)
    assert lds["counts"].tolist() == [[2414, 1, 68, 2414, 1, 68], [11238, 1004, 9096, 11238, 1004, V], [56, 3, 12, 56, 3, 12]]      # (image 1: V cuts its vertices short)
    four = run(maps, 4, 2 * LDS_CRACKS, Rr, V)
    same_bytes(four, dict(zip(NAMES, R.contours(maps, 4, 2 * LDS_CRACKS, Rr, V))), "global form, connectivity 4", NAMES)


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_agree():
    maps = np.zeros((3, 40, 75), np.int32)
    maps[0, :33, :70] = SHAPES["serpentine"][0]
    maps[1] = _random(40, 75, 11)
    maps[2, 20:29, 60:71] = _hole()
    C, Rr, V = 4000, 700, 2600                                       # image 1 holds more cracks than C: it takes none, its neighbours do
    whole = run(maps, 8, C, Rr, V)
    same_bytes(run(maps, 8, C, Rr, V, fill=0x00, ws_fill=0x7F), whole, "two calls", NAMES)
    for n in range(3):
        one = run(maps[n:n + 1], 8, C, Rr, V)
        same_bytes({k: v[0] for k, v in one.items()}, {k: v[n] for k, v in whole.items()}, n, NAMES)
    same_bytes(whole, dict(zip(NAMES, R.contours(maps, 8, C, Rr, V))), "the batch", NAMES)
    assert whole["counts"][1, 0] > C and whole["counts"][1, 1:].tolist() == [0] * 5 and whole["counts"][[0, 2], 3].tolist() == [2414, 56]
    larger = contours_call(np.ascontiguousarray(maps[:, ::-1]), 4, C, Rr, V)      # the same sizes, other contents in every array of the workspace
    same_bytes(run(maps, 8, C, Rr, V, before=(larger,)), whole, "after another call on the same workspace", NAMES)


def _blob_maps(N, H, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W]
    pred = np.zeros((N, H, W), np.float32)
    for n in range(N):
        for _ in range(7):
            cy, cx, r = rs.randint(0, H), rs.randint(0, W), rs.randint(3, 14)
            d2 = (yy - cy) ** 2 + (xx - cx) ** 2
            pred[n][(d2 < r * r) & (d2 >= (r // 2) ** 2 * (r % 2))] = 0.9      # discs and rings: the rings' holes are what fill_holes fills
    return pred


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [8, 4])
def test_round_trip_through_decode_polygons(conn):
    from camouflage_multimodal_amd import contours as C, decode_polygons, mask_instances
    H, W = 64, 96
    pred = torch.from_numpy(_blob_maps(3, H, W, 5)).cuda()
    labels = mask_instances(pred, 0.5, conn, 0, True)["labels"]
    assert not torch.equal(labels, mask_instances(pred, 0.5, conn, 0, False)["labels"])      # (a hole was filled)
    polys = C.encode_instance_polygons(labels, conn)
    host = labels.cpu().numpy()
    for n, image in enumerate(polys):
        assert sorted(image) == [int(v) for v in np.unique(host[n]) if v > 0] and len(image) >= 2
        for i, entry in image.items():
            assert len(entry["polygons"]) == 1 and entry["holes"] == [] and entry["area"] == int((host[n] == i).sum())
    back = decode_polygons([[(entry["polygons"], i) for i, entry in image.items()] for image in polys], H, W)
    assert torch.equal(back, labels)
    traced_ = C.trace_contours(labels, conn)
    same_bytes({k: v.cpu().numpy() for k, v in traced_.items()}, dict(zip(NAMES, R.contours(host, conn, *capacities(host)))), "trace_contours", NAMES)
    one = C.trace_contours(labels[0], conn, max_cracks=1200, max_rings=9, max_vertices=500)
    assert tuple(one["rings"].shape) == (1, 9, 5) and tuple(one["xy"].shape) == (1, 500, 2) and one["counts"].dtype == torch.int32


@pytest.mark.gpu
def test_encode_instance_polygons_takes_its_second_call():
    """More cracks than the default capacity: noise of three ids at 128 x 128 holds about 37 000."""
    from camouflage_multimodal_amd import contours as C
    maps = np.random.RandomState(3).randint(0, 4, (2, 128, 128)).astype(np.int32)
    maps[1] = 0
    maps[1, 5:9, 5:9] = 4
    t = torch.from_numpy(maps).cuda()
    first = C.trace_contours(t)["counts"].cpu().numpy()
    assert first[0, 0] > LDS_CRACKS and first[0, 1:].tolist() == [0] * 5 and first[1].tolist() == [16, 1, 4, 16, 1, 4]
    with pytest.raises(ValueError, match=rf"^image 0 holds {first[0, 0]} cracks and 0 were taken"):
        C.polygons_from_contours(**C.trace_contours(t))
    polys = C.encode_instance_polygons(t)
    assert polys[1] == {4: {"polygons": [[5, 5, 9, 5, 9, 9, 5, 9]], "holes": [], "area": 16}}
    assert {i: e["area"] for i, e in polys[0].items()} == {i: int((maps[0] == i).sum()) for i in (1, 2, 3)}
    ref = R.polygons(R.trace_image(maps[0], 8)[1])
    assert {i: (e["polygons"], e["holes"]) for i, e in polys[0].items()} == {i: (o, h) for i, (o, h) in ref.items()}
