"""COCO polygon annotations (include/camo_poly.h): the sequential numpy restatement tests/poly_ref.py against hand
facts, the host surface of camouflage_multimodal_amd/polygons.py (CPU), and the kernels against the restatement byte for byte (GPU).

Every raw call takes its buffers from tests/guarded.py and runs twice, with the memory around and inside the outputs and the
workspace filled with 0x00 and with 0xFF: nothing rests on memory the caller cleared, and the two runs must give the same bytes."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import poly_ref as P
import rle_ref as R
from raw_calls import BUILDERS, execute, same_bytes as _same

SHAPES = ((1, 1), (1, 70), (70, 1), (6, 7), (33, 70), (70, 33), (64, 64), (65, 129))
SQUARE, FULL, TRIANGLE = [1, 1, 4, 1, 4, 4, 1, 4], [0, 0, 7, 0, 7, 6, 0, 6], [-3, -2, 9, 2, 3, 9]
TRIANGLE_ROWS = ["1111000", "1111111", "1111111", "1111111", "0111111", "0111110"]
# Found by running tests/poly_ref.py's contracted_mask beside its polygon_mask over random polygons on a 0.2 grid: an edge that starts
# at a negative scaled coordinate where a + s t cancels.  (polygon, pixels by the definition, pixels when contracted)
ROUNDING = {(12, 12): [[5.0, 8.6, 6.8, 1.6, 14.0, -3.0], [-3.0, 6.8, 8.0, -4.0, 4.8, 16.4], [9.8, -1.4, 10.2, 13.8, -1.6, 0.2],
                       [14.2, -0.4, -3.6, 7.0, -0.6, 7.2, -4.2, 14.2]],
            (9, 20): [[19.0, 7.4, -0.4, 9.6, 17.6, -2.0, 11.6, 2.8], [13.4, 6.8, 9.8, 12.2, 0.2, 16.2, -2.8, -2.6], [20.2, 13.2, 0.6, 19.8, 18.6, 3.6, -1.2, 17.2]],
            (33, 70): [[53.2, 1.6, 27.6, 62.8, 2.8, -1.4], [5.2, 39.0, 4.8, 45.8, 58.0, 9.0]]}
ROUNDING_AREAS = {(12, 12): [(17, 18), (69, 70), (75, 76), (37, 38)], (9, 20): [(59, 58), (79, 80), (5, 4)], (33, 70): [(1206, 1208), (90, 91)]}


def _star(rng, cx, cy, r, k):
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.3 * r, r, k)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).reshape(-1).tolist()


def _walk(rng, H, W, k):
    p = np.cumsum(rng.normal(0, 0.2, (k, 2)) * (W, H), axis=0) + rng.uniform(0, 1, 2) * (W, H)
    return np.clip(p, -12, (W + 12, H + 12)).reshape(-1).tolist()


def _big_star():
    k = 200
    ang = np.arange(k) * 2 * np.pi / k
    rad = np.where(np.arange(k) % 2 == 0, 140.0, 90.0)
    return np.stack([250 + 1.6 * rad * np.cos(ang), 150 + rad * np.sin(ang)], axis=1).reshape(-1).tolist()


def _random_images(H, W, seed, N=2):
    rng = np.random.default_rng(seed)
    out = []
    for n in range(N):
        anns = []
        for a in range(3):
            k = int(rng.integers(3, 12))
            poly = _star(rng, rng.uniform(-2, W + 2), rng.uniform(-2, H + 2), 0.6 * max(H, W, 4), k) if a % 2 == 0 else _walk(rng, H, W, k)
            anns.append(([poly], int(rng.integers(1, 9))))
        out.append(anns)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (per image [(polygons, value)], H, W)"""
    kind, _, shape = name.partition("@")
    H, W = (int(v) for v in shape.split("x")) if shape else (33, 70)
    rng = np.random.default_rng(len(name) * 1009 + H * 131 + W)
    if kind == "random":
        per = _random_images(H, W, H * 131 + W)
    elif kind == "hand":                                             # 6 x 7: the facts of test_restatement_hand_facts, one value each
        per = [[([SQUARE], 1), ([[c + 0.5 for c in SQUARE]], 2), ([[3, 3]], 3), ([[3, 3, 5, 5]], 4), ([[2, 2, 2, 2, 2, 2]], 5), ([TRIANGLE], 6)],
               [([FULL], 2)], [([[1, 1, 5, 1, 5, 5, 1, 5, 1, 1]], 9)]]
    elif kind == "octants":                                          # every octant in both directions, horizontal and vertical edges
        ring = [(35 + 30 * np.cos(t), 16 + 14 * np.sin(t)) for t in np.arange(16) * 2 * np.pi / 16 + 0.1]
        flat = [c for p in ring for c in p]
        back = [c for p in reversed(ring) for c in p]
        box = [5.0, 3.0, 60.0, 3.0, 60.0, 29.0, 5.0, 29.0]
        per = [[([flat], 1)], [([back], 1)], [([box], 2), ([[box[i] for i in (6, 7, 4, 5, 2, 3, 0, 1)]], 1)],
               [([[2, 2, 66, 5, 60, 30, 4, 28]], 1), ([[10, 1, 14, 31, 30, 2, 33, 32, 50, 0]], 3)]]      # shallow, steep and zig-zag edges
    elif kind == "star":                                             # 300 x 500: 4688 words a plane, five passes of the scan; an edge of 6401 points
        per = [[([_big_star()], 2), ([[-400.0, 10.0, 880.0, 290.0, 100.0, 295.0]], 1)]]
    elif kind == "degenerate":                                       # zero-length edges, a bow-tie, overlapping and edge-sharing polygons
        a, b = [2, 2, 12, 2, 12, 10, 2, 10], [8, 2, 18, 2, 18, 10, 8, 10]
        c, d = [30, 4, 38, 4, 38, 12, 30, 12], [38, 4, 46, 4, 46, 12, 38, 12]
        per = [[([[2, 2, 2, 2, 10, 2, 10, 2, 10, 2, 10, 12, 2, 12, 2, 12]], 1), ([[20, 2, 40, 20, 40, 2, 20, 20]], 2)],
               [([a, b], 1), ([c, d], 2)], [([a + b], 1), ([c + d], 2)]]
    elif kind == "borders":                                          # outside on every side, across column W - 1, y clamped at 0 and at H
        per = [[([[-9, 5, -2, 5, -2, 20, -9, 20]], 1), ([[75, 5, 90, 5, 90, 20, 75, 20]], 2), ([[5, -9, 20, -9, 20, -1, 5, -1]], 3),
                ([[5, 36, 20, 36, 20, 50, 5, 50]], 4)],
               [([[60, 10, 80, 10, 80, 20, 60, 20]], 1), ([[50, -5, 75, -5, 75, 40, 50, 40]], 2), ([[3, -4, 9, 33, 15, -4]], 3)],
               [([[68.5, -3, 75, 36, 62, 36]], 5), ([[0, 0, 70, 0, 70, 33, 0, 33]], 1)]]
    elif kind == "margin":                                           # 6 x 7: coordinates at the margin and just inside it
        m = float(P.MARGIN)
        per = [[([[-m, -m, W + m, -m, W + m, H + m, -m, H + m]], 1)], [([[-m + 0.5, -m + 0.25, W + m - 0.5, 2.0, 3.0, H + m - 0.125]], 2)],
               [([[-m, 3.0, W + m, 3.0, W + m, 5.0, -m, 5.0]], 1), ([[3.0, -m, 5.0, -m, 5.0, H + m, 3.0, H + m]], 3)]]
    elif kind == "ties":                                             # multiples of 0.5 and 0.1, negative ones included: the roundings of step 1
        per = []
        for step in (0.5, 0.1, 0.1):
            anns = []
            for a in range(4):
                k = int(rng.integers(3, 9))
                pts = rng.integers(int(-8 / step), int((max(H, W) + 8) / step), (k, 2)) * step
                anns.append(([pts.reshape(-1).tolist()], a + 1))
            per.append(anns)
    elif kind == "rounding":                                         # masks that change when steps 1 and 2 are contracted into fused multiply-adds
        per = [[([p], i + 1) for i, p in enumerate(ROUNDING[(H, W)])]]
    elif kind == "mixed":                                            # 65 x 129: stars and walks of 3 .. 200 vertices, three polygons, no polygon
        per = [[([_star(rng, 60, 30, 40, 200)], 1), ([_walk(rng, H, W, 3)], 2), ([_walk(rng, H, W, 57)], 3), ([], 4)],
               [([_star(rng, 30, 20, 25, 7), _star(rng, 60, 40, 30, 31), _walk(rng, H, W, 12)], 5), ([_star(rng, 50, 30, 30, 5)], 2)],
               []]
        per[2] = list(reversed(per[1]))                              # the same overlapping annotations in the other order
    elif kind == "many":                                             # A annotations over three images
        A = H
        H, W = 33, 70
        per = [[] for _ in range(3)]
        for a in range(A):
            poly = [] if a % 17 == 5 else [_star(rng, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, 12), int(rng.integers(3, 7)))]
            per[int(rng.integers(0, 3))].append((poly, int(rng.integers(1, 40))))
    else:
        raise KeyError(name)
    return per, H, W


CASES = [f"random@{H}x{W}" for H, W in SHAPES] + ["hand@6x7", "octants", "star@300x500", "degenerate", "borders", "margin@6x7", "ties", "mixed@65x129",
                                                   "many@1x0", "many@300x0", "rounding@12x12", "rounding@9x20", "rounding@33x70"]


@functools.lru_cache(maxsize=None)
def _reference(name):
    per, H, W = _case(name)
    arrays = P.arrays(per)
    labels, area = P.decode(*arrays, len(per), H, W)
    labels.setflags(write=False); area.setflags(write=False)
    return arrays, labels, area


def _raw_decode(arrays, N, H, W, fill):
    """camo_poly_decode with every buffer a guarded piece filled with `fill` -> {"labels", "ann_area"} as numpy arrays."""
    return execute(BUILDERS["camo_poly_decode"](arrays, N, H, W), fill)


def _both_fills(arrays, N, H, W, want, what):
    got = _raw_decode(arrays, N, H, W, 0x00)
    if want is not None:
        _same(got, want, (what, 0x00))
    _same(_raw_decode(arrays, N, H, W, 0xFF), got, (what, 0xFF))      # and two calls give the same bytes
    return got


# ---- CPU: the restatement, the host surface, the argument checks ----------------------------------------------------------------

def _rows(mask):
    return ["".join("1" if v else "0" for v in r) for r in mask]


def test_restatement_hand_facts():
    sq = P.polygon_mask(SQUARE, 6, 7)
    assert sq.sum() == 9 and sq[1:4, 1:4].all()
    half = P.polygon_mask([c + 0.5 for c in SQUARE], 6, 7)
    assert half.sum() == 9 and half[2:5, 2:5].all()
    assert P.polygon_mask(FULL, 6, 7).all()
    assert _rows(P.polygon_mask(TRIANGLE, 6, 7)) == TRIANGLE_ROWS
    for empty in ([3, 3], [3, 3, 5, 5], [2, 2, 2, 2, 2, 2]):
        assert not P.polygon_mask(empty, 6, 7).any()
    assert P.polygon_mask([1, 1, 5, 1, 5, 5, 1, 5, 1, 1], 8, 8).sum() == 16
    star = _big_star()                                               # (this file's 200-vertex star, with figures of its own)
    assert len(P.polygon_toggles(star, 300, 500)) == 10216 and P.polygon_mask(star, 300, 500).sum() == 63360


def test_rounding_cases_tell_a_contracted_kernel_from_the_definition():
    """Step 2's (int)(a + s t + 0.5) with a = -1, s = 2 / 12, t = 9 is 1; with the product and the sum fused it is 0.  Every polygon
    of the GPU cases "rounding@..." has another mask when steps 1 and 2 are contracted."""
    from fractions import Fraction
    s = np.float64(2) / np.float64(12)
    assert int(np.float64(-1) + s * np.float64(9) + 0.5) == 1 and int(float(Fraction(float(s)) * 9 - 1) + 0.5) == 0
    for (H, W), polys in ROUNDING.items():
        for poly, (want, fused) in zip(polys, ROUNDING_AREAS[(H, W)]):
            a, b = P.polygon_mask(poly, H, W), P.contracted_mask(poly, H, W)
            assert (a.sum(), b.sum()) == (want, fused) and (a != b).any(), poly
    assert (P.contracted_mask(SQUARE, 6, 7) == P.polygon_mask(SQUARE, 6, 7)).all()      # (the emulation itself, where nothing cancels)


def test_restated_rectangles_fill_the_closed_form():
    rng = np.random.default_rng(11)
    for _ in range(60):
        H, W = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        x0, x1 = np.sort(rng.integers(-4, W + 5, 2))
        y0, y1 = np.sort(rng.integers(-4, H + 5, 2))
        corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        if rng.integers(0, 2):
            corners.reverse()
        start = int(rng.integers(0, 4))
        poly = [float(c) for p in corners[start:] + corners[:start] for c in p]
        want = np.zeros((H, W), bool)
        want[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
        assert (P.polygon_mask(poly, H, W) == want).all(), (H, W, poly)


def test_restated_counts_equal_the_parity_of_the_toggles():
    rng = np.random.default_rng(12)
    coinciding = 0
    for _ in range(120):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        poly = rng.uniform(-5, 45, 2 * int(rng.integers(1, 9))).tolist()
        pos = P.polygon_toggles(poly, H, W)
        coinciding += len(np.unique(pos)) < len(pos)
        counts = P.toggle_counts(pos, H, W)
        assert counts.sum() == H * W and (counts[1:] > 0).all()
        assert (P.counts_mask(counts, H, W) == P.parity_mask(pos, H, W)).all(), poly
    assert coinciding >= 20


def test_restated_annotation_rules():
    a, b, c = [2, 2, 12, 2, 12, 10, 2, 10], [8, 2, 18, 2, 18, 10, 8, 10], [4, 6, 16, 6, 16, 14, 4, 14]
    H, W = 16, 20
    union = P.polygon_mask(a, H, W) | P.polygon_mask(b, H, W) | P.polygon_mask(c, H, W)
    labels, area = P.decode(*P.arrays([[([a, b, c], 3), ([], 7), ([a], 2)], [([b], 1)]]), 2, H, W)
    assert area.tolist() == [union.sum(), 0, 80, 80] and union.sum() == 16 * 8 + 12 * 4 < 3 * 80
    assert (labels[0] == np.where(union, 3, 0)).all() and (labels[1] == np.where(P.polygon_mask(b, H, W), 1, 0)).all()
    xy, po, apo, img, val = P.arrays([[([a], 1), ([b], 2), ([c], 3), ([a], 4), ([[np.nan, 1, 2, 3]], 5), ([[1, 1, W + 1024.5, 3]], 6)]])
    img[1], val[2] = 1, 0
    po = np.insert(po, 4, po[3]); apo[4:] += 1                        # annotation 3 gains a polygon without a vertex
    labels, area = P.decode(xy, po, apo, img, val, 1, H, W)
    assert area.tolist() == [80, -1, -1, -1, -1, -1] and (labels[0] == P.polygon_mask(a, H, W)).all()


def _coco():
    return {"images": [{"id": 7, "file_name": "b_cat.png", "height": 33, "width": 70}, {"id": 11, "file_name": "sub/a_owl.jpg", "height": 70, "width": 33}],
            "annotations": [{"id": 1, "image_id": 11, "iscrowd": 0, "segmentation": [[2, 2, 20, 2, 20, 30, 2, 30]]},
                            {"id": 2, "image_id": 7, "iscrowd": 0, "segmentation": {"size": [33, 70], "counts": [40, 60, 2210]}},
                            {"id": 3, "image_id": 7, "iscrowd": 1, "segmentation": {"size": [33, 70], "counts": [0, 2310]}},
                            {"id": 4, "image_id": 11, "segmentation": [[1, 40, 30, 40, 30, 60], [5, 5, 8, 5, 8, 8]]}]}


def test_coco_ground_truth(tmp_path):
    from camouflage_multimodal_amd import coco_ground_truth
    coco = _coco()
    got = coco_ground_truth(coco, ["a_owl", "b_cat.png"])
    assert got["sizes"] == [(70, 33), (33, 70)] and got["image_ids"] == {"a_owl": 11, "b_cat": 7} and got["crowd_skipped"] == 1
    assert got["segmentations"] == [[coco["annotations"][0]["segmentation"], coco["annotations"][3]["segmentation"]], [coco["annotations"][1]["segmentation"]]]
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(coco))
    assert coco_ground_truth(str(path), ["a_owl", "b_cat.png"]) == got
    assert coco_ground_truth(coco, ["sub/a_owl.jpg"])["image_ids"] == {"a_owl": 11}
    with pytest.raises(ValueError, match="no image named 'c_moth'"):
        coco_ground_truth(coco, ["a_owl", "c_moth"])
    twice = dict(coco, images=coco["images"] + [{"id": 12, "file_name": "other/a_owl.jpg", "height": 8, "width": 8}])
    with pytest.raises(ValueError, match="more than one image with the stem of 'a_owl'"):
        coco_ground_truth(twice, ["a_owl"])
    with pytest.raises(ValueError, match="more than one image with the stem of 'a_owl.png'"):
        coco_ground_truth(twice, ["a_owl.png"])
    assert coco_ground_truth(twice, ["other/a_owl.jpg", "b_cat"])["sizes"] == [(8, 8), (33, 70)]      # the file name as stated is not ambiguous
    with pytest.raises(ValueError, match="COCO annotations file"):
        coco_ground_truth({"images": []}, ["a_owl"])


def test_argument_errors_by_name_and_no_cpu_path(monkeypatch):
    from camouflage_multimodal_amd import _lib, decode_polygon_arrays, decode_polygons, decode_segmentations, polygons_to_rles
    from camouflage_multimodal_amd._lib import CamoError
    ok = [[1, 1, 4, 1, 4, 4]]
    far = [[1, 1, 8 + 1024.5, 1, 4, 4]]
    for anns, word in ((None, "per_image_annotations"), ([], "per_image_annotations"), ([5], "image 0: need a list"),
                       ([[ok], [[[1, 2, 3]]]], "image 1, annotation 0: a polygon with an odd number of coordinates, 3"),
                       ([[ok, [[]]]], "image 0, annotation 1: an empty polygon"), ([[[[1, 1, float("nan"), 3]]]], "image 0, annotation 0: a coordinate is not finite"),
                       ([[[[1, 1, float("inf"), 3]]]], "not finite"), ([[far]], "image 0, annotation 0: a coordinate lies more than 1024 pixels outside"),
                       ([[[[1, -1024.5, 2, 2]]]], "more than 1024 pixels outside"), ([[[[1, 1, 2, 8 + 1024.5]]]], "more than 1024 pixels outside"),
                       ([[(ok, 0)]], "image 0, annotation 0: the value must be"), ([[(ok, True)]], "value must be"), ([[(ok, 2 ** 31)]], "value must be"),
                       ([[5]], "image 0, annotation 0: need a list of polygons"), ([[[5.0, 6.0]]], "a polygon must be a flat list"),
                       ([[[["a", "b"]]]], "a polygon must be a flat list")):
        with pytest.raises(ValueError, match=word):
            decode_polygons(anns, 8, 8, "cpu")
    with pytest.raises(ValueError, match="image 12, annotation 0: an empty polygon"):
        decode_polygons([[ok], [[[]]]], 8, 8, "cpu", image_numbers=[3, 12])
    with pytest.raises(ValueError, match="image 0, annotation 0: a coordinate lies more than 1024"):      # inside before the scale, outside after it
        decode_polygons([[[[1, 1, 600, 1, 4, 4]]]], 8, 8, "cpu", scales=[(2.0, 1.0)])
    for scales, word in (([(1, 1), (1, 1)], "2 scales for 1 images"), ([(0, 1)], "the scale must be"), ([(1, 2, 3)], "the scale must be"), ([5], "the scale must be")):
        with pytest.raises(ValueError, match=word):
            decode_polygons([[ok]], 8, 8, "cpu", scales=scales)
    for H, W in ((0, 4), (4, -1), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="must be an integer >= 1"):
            decode_polygons([[ok]], H, W, "cpu")
    for limit, anns, word in (("POLY_MAX_ANNOTATIONS", [[ok, ok, ok]], "3 annotations exceed 2"), ("POLY_MAX_POLYGONS", [[ok + ok + ok]], "3 polygons exceed 2"),
                              ("POLY_MAX_VERTICES", [[ok]], "3 vertices exceed 2")):
        with monkeypatch.context() as mp:
            mp.setattr(_lib, limit, 2)
            with pytest.raises(ValueError, match=word):
                decode_polygons(anns, 8, 8, "cpu")
    with monkeypatch.context() as mp:                                  # one annotation whose planes alone exceed the limit cannot be split
        mp.setattr(_lib, "POLY_MAX_PLANE_WORDS", 5)
        with pytest.raises(ValueError, match="image 0, annotation 1: 3 polygons on 8 x 8 need more than 5 plane words"):
            decode_polygons([[ok, ok + ok + ok]], 8, 8, "cpu")
    with monkeypatch.context() as mp:
        from camouflage_multimodal_amd import polygons
        mp.setattr(polygons, "MAX_BOUNDARY_POINTS", 40)
        with pytest.raises(ValueError, match="boundary points, more than 40"):
            decode_polygons([[ok]], 8, 8, "cpu")
    for good in ([[ok]], [[(ok, 9)], []], [[[]]], [[]]):
        with pytest.raises(CamoError, match="no CPU fallback"):
            decode_polygons(good, 8, 8, "cpu")
    with pytest.raises(CamoError, match="no CPU fallback"):
        polygons_to_rles([ok, []], 8, 8, "cpu")
    with pytest.raises(ValueError, match="^annotation 1: an empty polygon"):
        polygons_to_rles([ok, [[]]], 8, 8, "cpu")
    rle = {"size": [8, 8], "counts": [4, 12, 48]}
    for segs, word in ((None, "per_image"), ([5], "image 0: need a list"), ([[ok, 5]], "image 0, annotation 1: a segmentation is a polygon list or an RLE dict"),
                       ([[rle, [[1, 2, 3]]]], "image 0, annotation 1: a polygon with an odd number"), ([[ok, {"size": [8, 9], "counts": [72]}]], r"image 0, annotation 1: size \[8, 9\]"),
                       ([[ok], [{"size": [8, 8], "counts": [4, 12, 47]}]], "image 1, annotation 0: the counts sum to 63"), ([[(rle, 0)]], "image 0, annotation 0: the value must be"),
                       ([[rle, far]], "image 0, annotation 1: a coordinate lies more than 1024")):
        with pytest.raises(ValueError, match=word):
            decode_segmentations(segs, 8, 8, "cpu")
    for good in ([[ok, rle]], [[(rle, 3)], []], [[]]):
        with pytest.raises(CamoError, match="no CPU fallback"):
            decode_segmentations(good, 8, 8, "cpu")
    xy, po, apo, img, val = P.arrays([[(ok, 1)]])
    for kw, word in ((dict(poly_off=[0, 4]), "poly_off must be non-decreasing from 0 to the number of vertices, 3"), (dict(poly_off=[0, 2, 1, 3], ann_poly_off=[0, 3]), "poly_off must be"),
                     (dict(ann_poly_off=[0, 2]), "ann_poly_off must be non-decreasing from 0 to the number of polygons, 1"), (dict(ann_value=[1, 2]), "need ann_poly_off of 2"),
                     (dict(N=0), "N must be"), (dict(H=0), "H must be")):
        a = dict(dict(xy=xy, poly_off=po, ann_poly_off=apo, ann_image=img, ann_value=val, N=1, H=8, W=8), **kw)
        with pytest.raises(ValueError, match=word):
            decode_polygon_arrays(a["xy"], a["poly_off"], a["ann_poly_off"], a["ann_image"], a["ann_value"], a["N"], a["H"], a["W"], "cpu")
    with pytest.raises(CamoError, match="no CPU fallback"):
        decode_polygon_arrays(xy, po, apo, img, val, 1, 8, 8, "cpu")


def test_match_keyword_errors_by_name(tmp_path):
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU.  The messages earlier tests pin
    stay word for word."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged
    from camouflage_multimodal_amd.instance_match import match_options
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img, ids = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, dtype=torch.int32)
    segs = [[[[1, 1, 9, 1, 9, 9]]]]
    three = 'match takes one of "gt_labels", "gt_rles" and "gt_segmentations", not two'
    for other in ({"gt_labels": ids}, {"gt_rles": [[]]}):
        with pytest.raises(ValueError, match=three):
            detect_camouflage_batch(m, img, device="cpu", instances=True, match=dict(other, gt_segmentations=segs))
    with pytest.raises(ValueError, match=three):
        detect_camouflage(m, img[0], device="cpu", instances=True, match={"gt_rles": [[]], "gt_segmentations": segs})
    with pytest.raises(ValueError, match=three):
        detect_camouflage_ragged(m, [np.zeros((8, 8, 3), np.uint8)], device="cpu", instances=True, match={"gt_labels": [ids[0]], "gt_segmentations": segs})
    with pytest.raises(ValueError, match=r'match\["gt_segmentations"\] must be a non-empty list'):
        detect_camouflage_batch(m, img, device="cpu", instances=True, match={"gt_segmentations": "polygons"})
    with pytest.raises(ValueError, match="match needs instances=True"):
        detect_camouflage_batch(m, img, device="cpu", match={"gt_segmentations": segs})
    with pytest.raises(ValueError, match="match must be None, True or a dict"):      # "gt_coco" belongs to the directory call alone
        detect_camouflage_batch(m, img, device="cpu", instances=True, match={"gt_coco": _coco()})
    with pytest.raises(ValueError, match='match takes "gt_coco" or one of'):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", instances=True, match={"gt_coco": _coco(), "gt_segmentations": segs})
    with pytest.raises(ValueError, match=r'match\["gt_coco"\] must be the path'):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", instances=True, match={"gt_coco": 5})
    # pinned by earlier tests
    with pytest.raises(ValueError, match='match takes "gt_labels" or "gt_rles", not both'):
        match_options({"gt_labels": ids, "gt_rles": [[]]})
    with pytest.raises(ValueError, match='match takes "gt_labels" or "gt_rles", not both'):
        match_options({"gt_labels": ids, "gt_rles": [[]], "gt_segmentations": segs})
    with pytest.raises(ValueError, match="match must be None, True or a dict"):
        match_options({"threshold": [0.5]})
    with pytest.raises(ValueError, match="match needs ground truth"):
        match_options(True, True, False)
    assert match_options({"gt_segmentations": segs}, True, False)["gt_segmentations"] is segs
    assert match_options(None) is None and set(match_options(True)) == {"thresholds", "gt_labels", "gt_rles", "max_gt", "gt_segmentations"}


def test_header_constants_and_symbols():
    import os
    import re
    from camouflage_multimodal_amd import _lib
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "camo_poly.h")).read(), flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    assert int(m["CAMO_POLY_MAX_ANNOTATIONS"]) == _lib.POLY_MAX_ANNOTATIONS == 65535 and int(m["CAMO_POLY_MAX_POLYGONS"]) == _lib.POLY_MAX_POLYGONS == 65535
    assert m["CAMO_POLY_MAX_VERTICES"] == "(1 << 20)" and _lib.POLY_MAX_VERTICES == 1 << 20
    assert m["CAMO_POLY_MAX_PLANE_WORDS"] == "(1 << 28)" and _lib.POLY_MAX_PLANE_WORDS == 1 << 28
    assert int(m["CAMO_POLY_MARGIN"]) == _lib.POLY_MARGIN == P.MARGIN == 1024 and _lib.ABI_VERSION == 13
    assert _lib.symbols("camo_poly.h") == ("camo_poly_decode_workspace_bytes", "camo_poly_decode")
    rle_text = open(os.path.join(ROOT, "include", "camo_rle.h")).read()
    assert "camo_poly.h" in rle_text and "polygon annotations (COCO's frPoly)," not in rle_text


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    ws = L.camo_poly_decode_workspace_bytes
    assert ws(1, 1, 1, 1, 0, 0) > 0 and ws(1, 1, 1, 1, 0, 0) % 256 == 0 and ws(3, 300, 500, 4, 20, 4000) >= 20 * 4 * 4688
    assert ws(1, 8, 8, 65535, 65535, 1 << 20) > 0 and ws(1, 8192, 8192, 1, 128, 3) > 0
    for bad in ((0, 8, 8, 1, 1, 4), (65536, 1, 1, 1, 1, 4), (1, 0, 8, 1, 1, 4), (1, 8, -1, 1, 1, 4), (1, 8192, 8193, 1, 1, 4), (1, 8, 8, 0, 1, 4), (1, 8, 8, 65536, 1, 4),
                (1, 8, 8, 1, -1, 4), (1, 8, 8, 1, 65536, 4), (1, 8, 8, 1, 1, -1), (1, 8, 8, 1, 1, (1 << 20) + 1), (1, 8192, 8192, 1, 129, 4)):
        assert ws(*bad) == 0, bad
    p, big = ctypes.c_void_p(0x1000), 1 << 40
    good = dict(xy=p, V=12, poff=p, P=3, aoff=p, img=p, val=p, A=2, N=2, H=8, W=8, labels=p, area=p, ws=p, nbytes=big)

    def decode(**kw):
        a = dict(good, **kw)
        return L.camo_poly_decode(a["xy"], a["V"], a["poff"], a["P"], a["aoff"], a["img"], a["val"], a["A"], a["N"], a["H"], a["W"], a["labels"], a["area"],
                                  a["ws"], a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=8192, W=8193), dict(A=0), dict(A=65536), dict(P=-1), dict(P=65536), dict(V=-1),
               dict(V=(1 << 20) + 1), dict(H=8192, W=8192, P=129), dict(xy=None), dict(poff=None), dict(aoff=None), dict(img=None), dict(val=None),
               dict(labels=None), dict(area=None), dict(ws=None), dict(xy=ctypes.c_void_p(0x1004)), dict(area=ctypes.c_void_p(0x1004)),
               dict(ws=ctypes.c_void_p(0x1080)), dict(nbytes=ws(2, 8, 8, 2, 3, 12) - 1), dict(nbytes=0)):
        assert decode(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()


# ---- GPU: the kernels against the restatement, byte for byte ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_decode_equals_the_restatement_bytewise(name):
    per, H, W = _case(name)
    arrays, labels, area = _reference(name)
    got = _both_fills(arrays, len(per), H, W, {"labels": labels, "ann_area": area}, name)
    if name == "hand@6x7":
        assert got["ann_area"].tolist() == [9, 9, 0, 0, 0, sum(r.count("1") for r in TRIANGLE_ROWS), 42, 16]
        assert _rows(got["labels"][0] == 6)[0] == "1111000" and (got["labels"][0][2:4, 2:4] == 6).all() and (got["labels"][1] == 2).all()
    if name == "star@300x500":
        assert got["ann_area"].tolist() == [63360, 68071]
    if name.startswith("rounding"):
        assert got["ann_area"].tolist() == [a for a, _ in ROUNDING_AREAS[(H, W)]]
    if name == "degenerate":
        assert got["ann_area"].tolist() == [80, 180, 128, 128, 72, 96]        # union across polygons, even-odd within one
    if name == "borders":
        assert got["ann_area"][:4].tolist() == [0, 0, 0, 0] and got["ann_area"][4] == 100 and got["ann_area"][5] == 20 * 33 and got["ann_area"][8] == 33 * 70
    if name == "margin@6x7":
        assert got["ann_area"][0] == 42 and got["ann_area"][2] == 14 and got["ann_area"][3] == 12
    if name == "mixed@65x129":
        assert got["ann_area"][3] == 0 and got["labels"][1].tobytes() == got["labels"][2].tobytes() and (got["ann_area"] >= 0).all()
    if name.startswith("many"):
        assert len(got["ann_area"]) == int(name[5:].split("x")[0]) and got["labels"].any()


@pytest.mark.gpu
def test_a_batch_is_its_images():
    per, H, W = _case("mixed@65x129")
    whole = _raw_decode(P.arrays(per), len(per), H, W, 0xFF)
    at = 0
    for n, anns in enumerate(per):
        if anns:
            one = _raw_decode(P.arrays([anns]), 1, H, W, 0xFF)
            _same(one, {"labels": whole["labels"][n:n + 1], "ann_area": whole["ann_area"][at:at + len(anns)]}, f"image {n}")
        at += len(anns)


@pytest.mark.gpu
def test_invalid_annotations_write_nothing_beside_valid_ones():
    H, W = 33, 70
    ok = [5, 5, 30, 5, 30, 25, 5, 25]
    nan, pinf, ninf = float("nan"), float("inf"), -float("inf")
    per = [[([ok], 3), ([[1, 1, nan, 3, 9, 9]], 9), ([ok, [1, 1, pinf, 3, 9, 9]], 9), ([[1, ninf, 2, 3, 9, 9]], 9), ([[1, 1, W + 1024.5, 3, 9, 9]], 9),
            ([[1, -1024.5, 20, 3, 9, 9]], 9), ([ok], 0), ([ok], -4), ([[40, 5, 60, 5, 60, 25]], 2)],
           [([ok], 5), ([ok], 9), ([ok], 9), ([[10, 10, 40, 10, 40, 30]], 1)]]
    xy, po, apo, img, val = P.arrays(per)
    img[-3], img[-2] = 2, -1                                           # images outside 0 .. N - 1
    po = np.append(po, po[-1])                                         # the last annotation's polygon is followed by one without a vertex ...
    extra = np.append(apo, apo[-1] + 1)                                # ... which is an annotation of its own
    img, val = np.append(img, 1).astype(np.int32), np.append(val, 9).astype(np.int32)
    want = P.decode(xy, po, extra, img, val, 2, H, W)
    got = _both_fills((xy, po, extra, img, val), 2, H, W, dict(zip(("labels", "ann_area"), want)), "invalid")
    assert got["ann_area"].tolist() == [500, -1, -1, -1, -1, -1, -1, -1, 190, 500, -1, -1, 300, -1]
    assert sorted(np.unique(got["labels"]).tolist()) == [0, 1, 2, 3, 5]


@pytest.mark.gpu
def test_offsets_that_are_not_monotone_stay_inside_the_arrays():
    """The results are unspecified; nothing may be read or written outside the buffers (the guards are checked in _raw_decode)."""
    per, H, W = _case("random@33x70")
    xy, po, apo, img, val = P.arrays(per)
    for bad_po, bad_apo in ((po[::-1].copy(), apo), (po, apo[::-1].copy()), (np.full_like(po, 2 ** 31 - 1), np.full_like(apo, -2 ** 31)),
                            (np.where(np.arange(len(po)) % 2, -5, po + 100).astype(np.int32), np.where(np.arange(len(apo)) % 2, 10 ** 6, apo).astype(np.int32))):
        for fill in (0x00, 0xFF):
            got = _raw_decode((xy, bad_po, bad_apo, img, val), len(per), H, W, fill)
            assert got["labels"].min() >= 0 and got["labels"].max() <= val.max() and (got["ann_area"] >= -1).all()


@pytest.mark.gpu
def test_decode_polygons_forms_values_scales_and_split(monkeypatch):
    from camouflage_multimodal_amd import _lib, decode_polygon_arrays, decode_polygons
    H, W = 33, 70
    a, b, c = [[5, 5, 30, 5, 30, 25, 5, 25]], [[20, 10, 50, 10, 50, 30, 20, 30]], [[40, 2, 60, 2, 50, 20], [1, 28, 9, 28, 9, 32, 1, 32]]
    later = decode_polygons([[a, b, c], []], H, W)                      # values 1, 2, 3 in list order: the later one wins
    want = P.label_map([(a, 1), (b, 2), (c, 3)], H, W)
    assert later.dtype == torch.int32 and later.shape == (2, H, W) and later.is_cuda and later[0].cpu().numpy().tobytes() == want.tobytes() and not later[1].any()
    given, area = decode_polygons([[(a, 9), (b, 4), ([], 2)], [(c, 7)]], H, W, return_area=True)
    assert given[0].cpu().numpy().tobytes() == P.label_map([(a, 9), (b, 4)], H, W).tobytes() and given[1].cpu().numpy().tobytes() == P.label_map([(c, 7)], H, W).tobytes()
    assert area.dtype == torch.int64 and area.tolist() == [500, 600, 0, int((want == 3).sum())]
    arrays = P.arrays([[(a, 9), (b, 4), ([], 2)], [(c, 7)]])
    raw = decode_polygon_arrays(*arrays, 2, H, W)
    assert torch.equal(raw[0], given) and torch.equal(raw[1], area)
    native = [[2 * v if i % 2 == 0 else 3 * v for i, v in enumerate(p)] for p in c]      # the polygons at twice the width and three times the height
    scaled = decode_polygons([[a], [(native, 7)]], H, W, scales=[(1, 1), (0.5, 1.0 / 3.0)])
    third = [[v * 0.5 if i % 2 == 0 else v * (1.0 / 3.0) for i, v in enumerate(p)] for p in native]
    assert scaled[1].cpu().numpy().tobytes() == P.label_map([(third, 7)], H, W).tobytes()
    none, no_area = decode_polygons([[], []], H, W, return_area=True)
    assert none.shape == (2, H, W) and none.dtype == torch.int32 and none.is_cuda and not none.any() and no_area.shape == (0,)
    calls = []
    from camouflage_multimodal_amd import polygons
    inner = polygons.decode_polygon_arrays
    monkeypatch.setattr(polygons, "decode_polygon_arrays", lambda *args: (calls.append(len(args[3])), inner(*args))[1])
    monkeypatch.setattr(_lib, "POLY_MAX_PLANE_WORDS", 2 * ((H * W + 31) // 32))      # two polygons a call
    split, split_area = decode_polygons([[(a, 9), (b, 4), ([], 2)], [(c, 7)]], H, W, return_area=True)
    assert calls == [3, 1]
    assert torch.equal(split, given) and torch.equal(split_area, area)


@pytest.mark.gpu
def test_polygons_to_rles_keep_every_annotations_own_mask():
    from camouflage_multimodal_amd import decode_rles, polygons_to_rles, rle_area, string_to_counts
    H, W = 33, 70
    anns = [[[5, 5, 30, 5, 30, 25, 5, 25]], [[20, 10, 50, 10, 50, 30, 20, 30]], [], [[40, 2, 60, 2, 50, 20], [1, 28, 9, 28, 9, 32, 1, 32]], [[-9, -9, -2, -9, -2, -2]]]
    rles = polygons_to_rles(anns, H, W)
    assert len(rles) == 5 and all(r["size"] == [H, W] and isinstance(r["counts"], str) for r in rles)
    for polys, rle in zip(anns, rles):
        want = P.label_map([(polys, 1)], H, W) > 0
        assert string_to_counts(rle["counts"]).tolist() == R.mask_counts(want).tolist() and rle_area(rle) == want.sum()
        assert (decode_rles([[rle]], H, W)[0].cpu().numpy() > 0).tobytes() == want.tobytes()      # overlap included: each its own slot


@pytest.mark.gpu
def test_decode_segmentations_takes_both_kinds():
    from camouflage_multimodal_amd import counts_to_string, decode_segmentations
    H, W = 33, 70
    poly_a, poly_b = [[5, 5, 30, 5, 30, 25, 5, 25]], [[40, 2, 60, 2, 50, 20]]
    mask = np.zeros((H, W), bool)
    mask[8:20, 25:45] = True
    text = {"size": [H, W], "counts": counts_to_string(R.mask_counts(mask))}
    listed = {"size": [H, W], "counts": R.mask_counts(mask).tolist()}
    got = decode_segmentations([[poly_a, text, poly_b], [(listed, 4), (poly_a, 2)], []], H, W)
    first = np.maximum(P.label_map([(poly_a, 1), (poly_b, 3)], H, W), np.where(mask, 2, 0)).astype(np.int32)
    second = np.maximum(P.label_map([(poly_a, 2)], H, W), np.where(mask, 4, 0)).astype(np.int32)
    assert got.shape == (3, H, W) and got.dtype == torch.int32 and not got[2].any()
    assert got[0].cpu().numpy().tobytes() == first.tobytes() and got[1].cpu().numpy().tobytes() == second.tobytes()
    assert torch.equal(decode_segmentations([[text]], H, W)[0], torch.from_numpy(np.where(mask, 1, 0).astype(np.int32)).cuda())
