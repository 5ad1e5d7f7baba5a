"""Object instances of a predicted mask (include/camo_instances.h) against tests/instances_ref.py.

PARITY UNPINNED: the header is the definition and the numpy restatement (a flood fill) the checker.  CPU tests hold the restatement
to scipy.ndimage where that is installed (label, binary_fill_holes, find_objects, sum), the host ratios to hand values and the
argument checks to the header.  GPU tests hold the kernels to the restatement BYTE FOR BYTE -- labels, clean, table and counts are
integers and the header leaves nothing open -- for connectivity 4 and 8, with and without hole filling; two calls the same bytes; a
batch the rows of its images; a channel of [N, 3, H, W] read in place.

The cases are the smallest at which the kernels can go wrong; the labelling tile is 32 x 32 and a raster block takes 1024 pixels:
one pixel, one row, one column, one pixel more than a tile, no multiple of a tile, several tiles and more than one raster block.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import instances_ref as R
from conftest import ROOT

SHAPES = ((1, 1), (1, 70), (70, 1), (33, 33), (45, 70), (64, 96))
MODES = [(c, f) for c in (4, 8) for f in (False, True)]


def _values(mask, seed):
    """A probability map whose binarisation at 0.5 is ``mask``: (0.5, 1] on it, [0, 0.5) elsewhere, so Sq has something to sum."""
    u = np.random.RandomState(seed).uniform(0, 1, mask.shape).astype(np.float32)
    return np.where(mask, np.float32(0.55) + np.float32(0.45) * u, np.float32(0.45) * u).astype(np.float32)


def _ring(m, y0, x0, y1, x1):
    m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (pred fp32 [N, H, W], threshold); never written to."""
    thr = 0.5
    kind, _, arg = name.partition(":")
    if kind in ("empty", "full", "checker"):
        H, W = (int(v) for v in arg.split("x"))
        yy, xx = np.mgrid[:H, :W]
        mask = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool), "checker": (yy + xx) % 2 == 0}[kind]
        pred = _values(mask, H * 131 + W)[None]
    elif kind == "noise":                                        # pred uniform, threshold 1 - density
        shape, density = arg.split("@")
        H, W = (int(v) for v in shape.split("x"))
        thr = 1.0 - float(density)
        pred = np.random.RandomState(H * 977 + W + int(float(density) * 10)).uniform(0, 1, (1, H, W)).astype(np.float32)
    elif kind == "corner":                                       # two squares touching at a corner, which is a tile corner too
        m = np.zeros((45, 70), bool)
        m[20:32, 20:32] = True
        m[32:44, 32:44] = True
        pred = _values(m, 1)[None]
    elif kind == "gap":                                          # a one-pixel wall without its corner: the inside meets the outside
        m = np.zeros((45, 70), bool)                             # diagonally only -- a hole at 8 (background 4), none at 4
        _ring(m, 10, 10, 40, 50)
        m[10, 10] = False
        pred = _values(m, 2)[None]
    elif kind == "border":                                       # a C closed by the image's first column: its inside is no hole;
        m = np.zeros((45, 70), bool)                             # and a whole ring lying on the last row and column, whose inside is one
        m[5, 0:26] = m[20, 0:26] = True
        m[5:21, 25] = True
        _ring(m, 30, 50, 44, 69)
        pred = _values(m, 3)[None]
    elif kind == "nested":                                       # a ring in a ring, an island in the inner hole
        m = np.zeros((64, 96), bool)
        _ring(m, 4, 6, 60, 90)
        _ring(m, 14, 20, 50, 76)
        m[30:35, 40:50] = True
        pred = _values(m, 4)[None]
    elif kind == "serpentine":                                   # one pixel wide over 128 x 160: every other row, joined at alternate ends
        m = np.zeros((128, 160), bool)
        m[0::2] = True
        for i, r in enumerate(range(1, 127, 2)):
            m[r, 159 if i % 2 == 0 else 0] = True
        pred = _values(m, 5)[None]
    elif kind == "blobs":                                        # areas 4, 6 and 9, apart
        m = np.zeros((33, 33), bool)
        m[2:4, 2:4] = True
        m[10:12, 20:23] = True
        m[28:31, 30:33] = True
        pred = _values(m, 6)[None]
    elif kind == "special":                                      # NaN, +inf and -inf: scattered over noise, and inside a solid block
        rs = np.random.RandomState(7)
        pred = rs.uniform(0, 1, (1, 45, 70)).astype(np.float32)
        pred[0, 8:30, 8:40] = 0.8
        for v in (np.nan, np.inf, -np.inf):
            ys, xs = rs.randint(0, 45, 40), rs.randint(0, 70, 40)
            pred[0, ys, xs] = v
        pred[0, 12, 12], pred[0, 15, 20:23], pred[0, 20, 30] = np.nan, -np.inf, np.inf
    elif kind == "batch":                                        # N = 3, different content; foreground in every image's last row and last
        rs = np.random.RandomState(8)                            # column and in the next image's first row and first column
        masks = rs.uniform(0, 1, (3, 33, 40)) < np.array([0.3, 0.6, 0.45])[:, None, None]
        masks[:, -1, :] = True
        masks[:, :, -1] = True
        masks[1:, 0, :] = True
        masks[1:, :, 0] = True
        masks[0, 0, :] = False
        pred = np.stack([_values(m, 9 + i) for i, m in enumerate(masks)])
    else:
        raise KeyError(name)
    pred.setflags(write=False)
    return pred, thr


@functools.lru_cache(maxsize=None)
def _ref(name, connectivity, fill, min_area=0, max_instances=64):
    pred, thr = _case(name)
    out = R.instances(pred, thr, connectivity, min_area, fill, max_instances)
    for a in out:
        a.setflags(write=False)
    return out


def _device(pred, thr, connectivity, fill, min_area=0, max_instances=64):
    from camouflage_multimodal_amd import mask_instances
    t = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.array(pred)).cuda()
    out = mask_instances(t, thr, connectivity, min_area, fill, max_instances)
    assert out["labels"].dtype == torch.int32 and out["clean_mask"].dtype == torch.bool and out["table"].dtype == torch.int64 \
        and out["counts"].dtype == torch.int32 and all(v.is_cuda for v in out.values())
    return (out["labels"].cpu().numpy(), out["clean_mask"].cpu().numpy().astype(np.uint8), out["table"].cpu().numpy(),
            out["counts"].cpu().numpy())


def _same(got, want, what):
    for g, w, part in zip(got, want, ("labels", "clean", "table", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {part} differs at {len(bad)} places, first {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}; "
                                 f"counts {got[3].tolist()} against {want[3].tolist()}")


STRUCTURED = ("corner", "gap", "border", "nested", "serpentine", "blobs", "special", "batch")
GRID = [f"{k}:{h}x{w}" for h, w in SHAPES for k in ("empty", "full", "checker")] + \
       [f"noise:{h}x{w}@{d}" for h, w in SHAPES for d in (0.3, 0.5, 0.7)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------

def test_header_constants_and_abi_version():
    from camouflage_multimodal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "camo_instances.h")).read()
    assert "PARITY UNPINNED" in hdr and "tests/instances_ref.py" in hdr

    def macro(name):
        v = re.search(rf"#define {name} (\S+(?: << \d+\))?)", hdr).group(1)
        m = re.fullmatch(r"\(1 << (\d+)\)", v)
        return 1 << int(m.group(1)) if m else int(v)
    assert _lib.INST_FIELDS == macro("CAMO_INST_FIELDS") == R.FIELDS == 8
    assert _lib.INST_COUNTS == macro("CAMO_INST_COUNTS") == R.COUNTS == 4
    assert _lib.INST_MAX_ROWS == macro("CAMO_INST_MAX_ROWS") == 1 << 24
    assert _lib.ABI_VERSION == 13 and "#define CAMO_ABI_VERSION 13" in open(os.path.join(ROOT, "include", "camo_fusion.h")).read()
    assert _lib.symbols("camo_instances.h") == ("camo_instances_workspace_bytes", "camo_instances")


def test_reference_hand_cases():
    """What the structured cases are built to show, on the restatement itself."""
    count = lambda name, c, f, a=0: _ref(name, c, f, a)[3][0].tolist()
    assert count("corner", 4, False) == [2, 0, 0, 288] and count("corner", 8, False) == [1, 0, 0, 288]
    assert count("gap", 8, True)[2] == 1 and count("gap", 4, True)[2] == 0                 # a hole at 8, none at 4
    assert count("gap", 8, True)[3] == 31 * 41 - 1 and count("gap", 4, True)[3] == count("gap", 4, False)[3]
    assert count("border", 8, True)[2] == 1 and count("border", 4, True)[2] == 1           # the whole ring's inside only
    assert count("nested", 8, False)[0] == 3 and count("nested", 8, True)[:3] == [1, 0, 2] and count("nested", 8, True)[3] == 57 * 85
    assert count("serpentine", 4, False)[0] == 1 and count("serpentine", 8, True)[:3] == [1, 0, 0]
    assert count("checker:45x70", 4, False)[0] == 1575 and count("checker:45x70", 8, False)[0] == 1
    # 8: the background is 4-connected, every background pixel off the border is a hole of its own; 4: it is 8-connected and one component
    assert count("checker:45x70", 8, True) == [1, 0, 43 * 68 // 2, 45 * 70 // 2 + 43 * 68 // 2] and count("checker:45x70", 4, True) == [1575, 0, 0, 1575]
    assert count("blobs", 8, False, 5)[:2] == [2, 1] and count("blobs", 8, False, 6)[:2] == [2, 1] and count("blobs", 8, False, 7)[:2] == [1, 2]
    lab, clean, table, counts = _ref("blobs", 8, False, 6)
    assert table[0, 0].tolist()[:5] == [6, 20, 10, 22, 11] and table[0, 1].tolist()[:5] == [9, 30, 28, 32, 30] and not table[0, 2:].any()
    assert table[0, 0, 5] == 2 * (20 + 21 + 22) and table[0, 0, 6] == 3 * (10 + 11) and set(np.unique(lab)) == {0, 1, 2}
    assert count("empty:1x1", 8, True) == [0, 0, 0, 0] and count("full:1x1", 4, True) == [1, 0, 0, 1]


@pytest.mark.parametrize("name", GRID[2::3] + list(STRUCTURED))
def test_reference_against_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    pred, thr = _case(name)
    cross, full = ndi.generate_binary_structure(2, 1), np.ones((3, 3), bool)
    for conn, fill in MODES:
        labels, clean, table, counts = _ref(name, conn, fill)
        for i, p in enumerate(pred):
            with np.errstate(invalid="ignore"):
                mask = p > np.float32(thr)
            if fill:                                               # (the structure is the BACKGROUND's connectivity: the complement)
                filled = ndi.binary_fill_holes(mask, structure=cross if conn == 8 else full)
                assert counts[i, 2] == ndi.label(filled & ~mask, structure=cross if conn == 8 else full)[1]
                mask = filled
            lab, n = ndi.label(mask, structure=full if conn == 8 else cross)
            assert n == counts[i, 0] and np.array_equal(lab, labels[i]) and np.array_equal(clean[i], mask.astype(np.uint8))
            assert counts[i, 1] == 0 and counts[i, 3] == mask.sum()
            k = min(n, table.shape[1])
            if k:
                idx = np.arange(1, k + 1)
                yy, xx = np.mgrid[:p.shape[0], :p.shape[1]]
                boxes = ndi.find_objects(lab)[:k]
                assert np.array_equal(table[i, :k, 0], ndi.sum(np.ones_like(lab), lab, idx).astype(np.int64))
                assert table[i, :k, 1:5].tolist() == [[b[1].start, b[0].start, b[1].stop - 1, b[0].stop - 1] for b in boxes]
                assert np.array_equal(table[i, :k, 5], ndi.sum(xx, lab, idx).astype(np.int64))
                assert np.array_equal(table[i, :k, 6], ndi.sum(yy, lab, idx).astype(np.int64))
                assert np.array_equal(table[i, :k, 7], ndi.sum(R.quantise(p), lab, idx).astype(np.int64))
            assert not table[i, k:].any()


def test_instance_records_arithmetic():
    from camouflage_multimodal_amd import instance_records
    table = [[[6, 20, 10, 22, 11, 126, 63, 1000], [1, 0, 0, 0, 0, 0, 0, 255], [0] * 8],
             [[7, 1, 2, 3, 4, 15, 22, 0], [3, 5, 5, 7, 5, 18, 15, 383], [2, 9, 9, 9, 10, 18, 19, 1]]]
    counts = [[2, 1, 0, 7], [5, 0, 3, 40]]
    for tab, cnt in ((table, counts), (torch.tensor(table), torch.tensor(counts, dtype=torch.int32))):
        a, b = instance_records(tab, cnt, 10, 8)
        assert [r["id"] for r in a["instances"]] == [1, 2] and a["count"] == 2 and a["truncated"] is False
        assert (a["dropped"], a["holes"], a["pixels"], a["coverage"]) == (1, 0, 7, 7 / 80)
        first, second = a["instances"]
        assert first == {"id": 1, "area": 6, "box": (20, 10, 22, 11), "centroid": (126 / 6, 63 / 6), "score": 1000 / (255 * 6)}
        assert second["score"] == 1.0 and second["centroid"] == (0.0, 0.0) and second["box"] == (0, 0, 0, 0)
        assert b["count"] == 5 and b["truncated"] is True and [r["id"] for r in b["instances"]] == [1, 2, 3] and b["holes"] == 3
        assert b["instances"][0]["score"] == 0.0 and b["instances"][1]["centroid"] == (6.0, 5.0)
        assert b["instances"][1]["score"] == 383 / 765 and b["instances"][2]["centroid"] == (9.0, 9.5) and b["instances"][2]["score"] == 1 / 510
    assert instance_records(torch.zeros(1, 4, 8, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int32), 3, 3) == \
        [{"instances": [], "count": 0, "truncated": False, "dropped": 0, "holes": 0, "pixels": 0, "coverage": 0.0}]
    with pytest.raises(ValueError, match="table holds 2 images, counts 1"):
        instance_records(table, counts[:1], 10, 8)


def test_argument_errors_by_name_and_no_cpu_path():
    from camouflage_multimodal_amd import (RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_ragged, detect_instances,
                                           mask_instances)
    from camouflage_multimodal_amd._lib import CamoError
    p = torch.zeros(2, 4, 4)
    for fn in (mask_instances, detect_instances):
        for kw, word in (({"connectivity": 6}, "connectivity"), ({"connectivity": True}, "connectivity"), ({"min_area": -1}, "min_area"),
                         ({"min_area": 2.5}, "min_area"), ({"max_instances": 0}, "max_instances"), ({"max_instances": (1 << 23) + 1}, "max_instances"),
                         ({"threshold": float("nan")}, "threshold"), ({"threshold": float("inf")}, "threshold"), ({"threshold": "0.5"}, "threshold")):
            with pytest.raises(ValueError, match=word):
                fn(p, **kw)
        with pytest.raises(ValueError, match=r"need pred \[N, H, W\]"):
            fn(torch.zeros(2, 3, 4, 4))
        with pytest.raises(ValueError, match=r"need pred \[N, H, W\]"):
            fn(torch.zeros(0, 4))
        with pytest.raises(CamoError, match="pred is on cpu"):     # good arguments, a CPU tensor: no fallback
            fn(p)
        with pytest.raises(CamoError, match="pred is on cpu"):
            fn(p[0], 0.25, 4, 3, True, 7)
    m = RegionGraphGNN().eval()
    img = torch.zeros(1, 16, 16, 3)
    for kw, word in (({"connectivity": 5}, "connectivity"), ({"min_area": -2}, "min_area"), ({"threshold": float("nan")}, "threshold")):
        with pytest.raises(ValueError, match=word):
            detect_camouflage_batch(m, img, instances=True, device="cpu", **kw)
        with pytest.raises(ValueError, match=word):
            detect_camouflage(m, img[0], instances=True, device="cpu", **kw)
        with pytest.raises(ValueError, match=word):
            detect_camouflage_ragged(m, [np.zeros((8, 8, 3), np.uint8)], instances=True, device="cpu", **kw)
    with pytest.raises(CamoError):
        detect_camouflage_batch(m, img, instances=True, min_area=4, fill_holes=True, connectivity=4, device="cpu")
    with pytest.raises(CamoError):
        detect_camouflage(m, img[0], instances=True, device="cpu")
    with pytest.raises(CamoError):
        detect_camouflage_ragged(m, [np.zeros((8, 8, 3), np.uint8)], instances=True, device="cpu")


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    ws = L.camo_instances_workspace_bytes
    assert ws(1, 1, 1) > 0 and ws(1, 1, 1) % 256 == 0 and ws(16, 256, 256) >= 16 * 256 * 256 * 13 and ws(2, 64, 96) > ws(1, 64, 96)
    assert ws(0, 8, 8) == 0 and ws(-1, 8, 8) == 0 and ws(1, 0, 8) == 0 and ws(1, 8, 0) == 0 and ws(65536, 1, 1) == 0 and ws(65535, 1, 1) > 0
    assert ws(1, 8192, 8192) > 0 and ws(1, 8192, 8193) == 0 and ws(16, 8192, 8192) > 0 and ws(17, 8192, 8192) == 0
    p, big = ctypes.c_void_p(0x1000), 1 << 40
    good = dict(pred=p, stride=64, thr=0.5, N=2, H=8, W=8, conn=8, min_area=0, fill=0, max_inst=4, labels=p, clean=p, table=p, counts=p, ws=p, nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return L.camo_instances(a["pred"], a["stride"], a["thr"], a["N"], a["H"], a["W"], a["conn"], a["min_area"], a["fill"], a["max_inst"], a["labels"],
                                a["clean"], a["table"], a["counts"], a["ws"], a["nbytes"], None)
    bad = [dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=8192, W=8193), dict(N=17, H=8192, W=8192, stride=1 << 26), dict(conn=6), dict(conn=0),
           dict(min_area=-1), dict(max_inst=0), dict(max_inst=(1 << 23) + 1), dict(stride=63), dict(thr=float("nan")), dict(thr=float("inf")),
           dict(thr=float("-inf")), dict(pred=None), dict(labels=None), dict(clean=None), dict(table=None), dict(counts=None), dict(ws=None),
           dict(table=ctypes.c_void_p(0x1004)), dict(ws=ctypes.c_void_p(0x1080)), dict(nbytes=ws(2, 8, 8) - 1), dict(nbytes=0)]
    for kw in bad:
        assert call(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", GRID + [s for s in STRUCTURED if s != "batch"])
def test_kernels_equal_the_reference_bytewise(name):
    pred, thr = _case(name)
    t = torch.from_numpy(np.array(pred)).cuda()
    for conn, fill in MODES:
        _same(_device(t, thr, conn, fill), _ref(name, conn, fill), f"{name} connectivity {conn} fill {fill}")


@pytest.mark.gpu
def test_min_area_at_below_and_above_a_components_area():
    pred, thr = _case("blobs")                                       # areas 4, 6, 9
    for a in (0, 4, 5, 6, 7, 9, 10):
        _same(_device(pred, thr, 8, False, a), _ref("blobs", 8, False, a), f"min_area {a}")
    got = _device(pred, thr, 8, False, 7)
    assert got[3][0].tolist() == [1, 2, 0, 9] and got[2][0, 0, :5].tolist() == [9, 30, 28, 32, 30]
    name = "noise:45x70@0.5"                                         # many sizes at once, with the holes filled first
    pred, thr = _case(name)
    areas = sorted(set(_ref(name, 4, True)[2][0, :, 0].tolist()) - {0})
    a = areas[len(areas) // 2]
    for conn, fill in MODES:
        for m in (a - 1, a, a + 1):
            _same(_device(pred, thr, conn, fill, m), _ref(name, conn, fill, m), f"{name} connectivity {conn} fill {fill} min_area {m}")


@pytest.mark.gpu
def test_truncated_table_and_the_second_call():
    from camouflage_multimodal_amd import detect_instances, instance_records
    name = "checker:45x70"                                           # 1575 one-pixel components at 4: K >> max_instances
    pred, thr = _case(name)
    t = torch.from_numpy(np.array(pred)).cuda()
    for rows in (1, 64, 1575, 1600):
        _same(_device(t, thr, 4, False, 0, rows), _ref(name, 4, False, 0, rows), f"{name} max_instances {rows}")
    labels, _, table, counts = _ref(name, 4, False, 0, 1575)
    assert counts[0, 0] == 1575 and labels.max() == 1575 and table[0, -1, 0] == 1
    from camouflage_multimodal_amd import mask_instances
    short = mask_instances(t, thr, 4)
    rec = instance_records(short["table"], short["counts"], 45, 70)[0]
    assert rec["truncated"] is True and rec["count"] == 1575 and len(rec["instances"]) == 64 and int(short["labels"].max()) == 1575
    out = detect_instances(t, thr, 4)
    assert tuple(out["table"].shape) == (1, 1575, 8) and np.array_equal(out["table"].cpu().numpy(), table)
    got = out["instances"][0]
    assert got["truncated"] is False and got["count"] == 1575 and [r["id"] for r in got["instances"]] == list(range(1, 1576))
    q = R.quantise(pred[0])
    ys, xs = np.nonzero(labels[0])
    for k in (0, 63, 64, 1574):
        r = got["instances"][k]
        assert r["area"] == 1 and r["box"] == (xs[k], ys[k], xs[k], ys[k]) and r["centroid"] == (float(xs[k]), float(ys[k]))
        assert r["score"] == int(q[ys[k], xs[k]]) / 255
    whole = detect_instances(t, thr, 8)                               # one component: no second call, the table as asked
    assert tuple(whole["table"].shape) == (1, 64, 8) and whole["instances"][0]["count"] == 1 and whole["instances"][0]["truncated"] is False


@pytest.mark.gpu
def test_filled_holes_are_summed_with_their_own_values():
    pred, thr = _case("nested")
    lab, clean, table, counts = _device(pred, thr, 8, True)
    q = R.quantise(pred[0])
    assert counts[0].tolist() == [1, 0, 2, 57 * 85] and table[0, 0, :5].tolist() == [57 * 85, 6, 4, 90, 60]
    assert table[0, 0, 7] == q[4:61, 6:91].sum() and table[0, 0, 7] > q[pred[0] > 0.5].sum()
    assert table[0, 0, 5] == 57 * sum(range(6, 91)) and table[0, 0, 6] == 85 * sum(range(4, 61))
    assert clean[0, 4:61, 6:91].all() and clean.sum() == 57 * 85 and (lab[0] == clean[0]).all()


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_are_the_same_bytes():
    pred, thr = _case("batch")
    t = torch.from_numpy(np.array(pred)).cuda()
    for conn, fill in MODES:
        first = _device(t, thr, conn, fill, 3)
        _same(first, _ref("batch", conn, fill, 3), f"batch connectivity {conn} fill {fill}")
        again = _device(t, thr, conn, fill, 3)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
        for i in range(3):
            one = _device(t[i], thr, conn, fill, 3)
            for a, b in zip(one, first):
                assert a[0].tobytes() == b[i].tobytes(), (conn, fill, i)


@pytest.mark.gpu
def test_a_plane_is_read_in_place():
    from camouflage_multimodal_amd import mask_instances
    pred, thr = _case("batch")
    maps = torch.full((3, 3, 33, 40), float("nan")).cuda()
    maps[:, 0] = torch.from_numpy(np.array(pred)).cuda()
    plane = maps[:, 0]
    assert not plane.is_contiguous() and plane.stride(0) == 3 * 33 * 40
    for conn, fill in MODES:
        _same(_device(plane, thr, conn, fill), _ref("batch", conn, fill), f"plane connectivity {conn} fill {fill}")
    out = mask_instances(maps[:1, 0], thr)                           # N = 1 of a strided map; and a single [H, W]
    assert np.array_equal(out["labels"].cpu().numpy(), _ref("batch", 8, False)[0][:1])
    out = mask_instances(maps[2, 0], thr, 4, 0, True)
    assert np.array_equal(out["labels"].cpu().numpy(), _ref("batch", 4, True)[0][2:])
    half = mask_instances(plane.double(), thr)                       # another dtype is converted, not reinterpreted
    assert np.array_equal(half["table"].cpu().numpy(), _ref("batch", 8, False)[2])


@pytest.mark.gpu
def test_the_no_op_settings_give_the_threshold_mask():
    from camouflage_multimodal_amd import mask_instances
    for name in ("special", "noise:64x96@0.5", "batch"):
        pred, thr = _case(name)
        t = torch.from_numpy(np.array(pred)).cuda()
        for conn in (4, 8):
            out = mask_instances(t, thr, conn, 0, False)
            assert torch.equal(out["clean_mask"], t > thr) and torch.equal(out["labels"] > 0, t > thr)
            assert out["counts"][:, 3].tolist() == (t > thr).sum(dim=(1, 2)).tolist()


@pytest.mark.gpu
def test_device_argument_errors():
    from camouflage_multimodal_amd import mask_instances
    t = torch.zeros(2, 4, 4, device="cuda")
    for kw, word in (({"connectivity": 6}, "connectivity"), ({"min_area": -1}, "min_area"), ({"max_instances": 0}, "max_instances"),
                     ({"threshold": float("nan")}, "threshold")):
        with pytest.raises(ValueError, match=word):
            mask_instances(t, **kw)
    out = mask_instances(t, 0.5, 8, 0, True, 3)
    assert not out["labels"].any() and not out["table"].any() and not out["counts"].any() and tuple(out["table"].shape) == (2, 3, 8)
