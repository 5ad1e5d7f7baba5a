"""COCO run-length masks (include/camo_rle.h): the numpy restatement tests/rle_ref.py against plain loops and hand
cases, the host codec of camouflage_multimodal_amd/rle.py against it (CPU), and the kernels against the restatement byte for byte (GPU).

The GPU cases give the label maps directly as int32 tensors, so the kernels meet what camo_instances never writes: a new run at every
pixel, negative labels, INT32_MAX.  Every raw call places its outputs between guard bytes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rle_ref as R
from inst_match_ref import blocks as _blocks
from raw_calls import BUILDERS, execute, same_bytes as _same

SHAPES = ((1, 1), (1, 70), (70, 1), (33, 70), (70, 33), (64, 64), (65, 129))      # tiles, halo rows and segment boundaries are all crossed
FILL, SKEW = 0xA5, 8      # the outputs start from 0xA5 (rle_ref holds -1 entries, which 0xFF would let a missed store pass), 8-byte aligned and no more


def _crossing():
    """Id 3 ends column 4 and begins column 5: one run; id 2 ends column 9 and id 1 begins column 10: two."""
    m = np.zeros((70, 33), np.int64)
    m[60:, 4], m[:5, 5] = 3, 3
    m[66:, 9], m[:2, 10] = 2, 1
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (labels int32 [N, H, W], R)"""
    kind, _, shape = name.partition("@")
    H, W = (int(v) for v in shape.split("x")) if shape else (0, 0)
    if kind == "blocks":
        lab = _blocks(H, W, 5, H * 131 + W, 3)[None]
    elif kind == "background":
        lab = np.zeros((1, H, W), np.int64)
    elif kind == "one_id":
        lab = np.full((1, H, W), 7, np.int64)
    elif kind == "crossing":
        lab = _crossing()[None]
    elif kind in ("checkerboard", "checkerboard_short"):
        y, x = np.mgrid[0:65, 0:129]
        lab = ((x + y) % 2)[None]                                      # H is odd: the last pixel of a column differs from the first of the next
        return lab.astype(np.int32), 65 * 129 - (kind == "checkerboard_short")
    elif kind == "extreme":
        lab = np.array([-2 ** 31, -1, 0, 2 ** 31 - 1, 7, 2 ** 31 - 2])[_blocks(33, 70, 5, 9, 3)][None]
    elif kind == "batch":
        lab = np.stack([_blocks(70, 33, 4, 40 + n, 2 + n) for n in range(5)])
    else:
        raise KeyError(name)
    lab = lab.astype(np.int32)
    return lab, max(int(R.runs_batch(lab, 1)["counts"][:, 0].max()) + 3, 8)


CASES = [f"{k}@{H}x{W}" for H, W in SHAPES for k in ("blocks", "background", "one_id")] + ["crossing", "checkerboard", "checkerboard_short", "extreme", "batch"]


def _raw_runs(labels, R_):
    """camo_rle_runs on guarded buffers (tests/raw_calls.py), the workspace 0xFF -> the outputs as numpy arrays."""
    return execute(BUILDERS["camo_rle_runs"](labels, R_), FILL, ws_fill=0xFF, skew=SKEW)


def _raw_decode(cnts, ann_off, ann_image, ann_value, N, H, W):
    return execute(BUILDERS["camo_rle_decode"]((cnts, ann_off, ann_image, ann_value), N, H, W), FILL, ws_fill=0xFF, skew=SKEW)


def _annotation_arrays(per_image):
    """[[(counts, value), ...] per image] -> (cnts, ann_off, ann_image, ann_value)"""
    cnts, off, img, val = [], [0], [], []
    for n, anns in enumerate(per_image):
        for c, v in anns:
            cnts += [int(x) for x in c]
            off.append(len(cnts)); img.append(n); val.append(v)
    return cnts, off, img, val


# ---- CPU: the restatement, the codec, the argument checks -------------------------------------------------------------------

def test_restated_runs_equal_a_loop_over_the_positions():
    for H, W, seed in ((5, 7, 0), (7, 5, 1), (5, 7, 2), (7, 5, 3)):
        lab = _blocks(H, W, 3, seed, 2).astype(np.int32)
        runs, counts = R.runs_image(lab, 64)
        want = R.runs_by_loop(lab)
        assert counts.tolist() == [len(want), len(want)] and [tuple(r) for r in runs[:len(want)].tolist()] == want and not runs[len(want):].any()
        short, c2 = R.runs_image(lab, 3)
        assert c2.tolist() == [len(want), 3] and [tuple(r) for r in short.tolist()] == want[:3]
    cross = _crossing()
    runs, counts = R.runs_image(cross, 16)
    assert [tuple(r) for r in runs[:counts[0]].tolist()] == [(0, 0), (4 * 70 + 60, 3), (5 * 70 + 5, 0), (9 * 70 + 66, 2), (10 * 70, 1), (10 * 70 + 2, 0)]


def test_restated_decode_of_encode_is_the_map():
    for H, W, seed in ((5, 7, 4), (7, 5, 5), (33, 70, 6)):
        lab = _blocks(H, W, 4, seed, 2).astype(np.int32)
        per_id = R.label_counts(lab)
        assert set(per_id) == set(np.unique(lab[lab > 0]).tolist())
        for i, c in per_id.items():
            assert c.sum() == H * W and (c[1:] > 0).all() and (R.counts_mask(c, H, W) == (lab == i)).all()
        cnts, off, img, val = _annotation_arrays([[(c, i) for i, c in per_id.items()]])
        back, sums = R.decode(cnts, off, img, val, 1, H, W)
        assert (back[0] == lab).all() and (sums == H * W).all()


def test_hand_strings():
    from camouflage_multimodal_amd import counts_to_string, string_to_counts
    for cnts, text in (([4], "4"), ([0, 4], "04"), ([15], "?"), ([16], "`0"), ([31], "o0"), ([1, 2, 3, 1], "123O")):
        assert R.to_string(cnts) == text and R.from_string(text) == cnts
        assert counts_to_string(cnts) == text and string_to_counts(text).tolist() == cnts
    assert counts_to_string([]) == "" and string_to_counts("").tolist() == []
    assert string_to_counts(b"123O").tolist() == [1, 2, 3, 1] and string_to_counts("123O").dtype == np.int64


def test_codec_round_trip_with_negative_deltas():
    from camouflage_multimodal_amd import counts_to_string, string_to_counts
    rng = np.random.default_rng(7)
    negative = 0
    for trial in range(60):
        n = int(rng.integers(1, 50))
        cnts = rng.integers(0, 1 << int(rng.integers(1, 27)), n)
        if trial % 3 == 0:
            cnts[rng.integers(0, n)] = (1 << 26) - 1
        if trial % 4 == 0 and n > 4:
            cnts[4], cnts[2] = 0, (1 << 26) - 1                       # cnts[4] - cnts[2] = -(2^26 - 1): the most negative delta
        text = counts_to_string(cnts)
        assert text == R.to_string(cnts.tolist()) and string_to_counts(text).tolist() == cnts.tolist() == R.from_string(text)
        assert n <= len(text) <= 6 * n                               # at most 6 groups below 2^26
        negative += any(c < a for a, c in zip(cnts[1:-2], cnts[3:]))
    assert negative >= 30                                            # (the lists do hold negative deltas)


def test_rles_from_runs_hand_cases():
    from camouflage_multimodal_amd import rle_area, rles_from_runs, string_to_counts
    # 2 x 3, positions 0 .. 5: id 2 owns position 0, id 1 owns the last one, id 3 is absent
    runs = np.array([[[0, 2], [1, 0], [3, 2], [4, 1], [0, 0], [0, 0]]], np.int32)
    counts = np.array([[4, 4]], np.int32)
    out, = rles_from_runs(runs, counts, 2, 3)
    assert list(out) == [1, 2] and 3 not in out and all(v["size"] == [2, 3] for v in out.values())
    assert string_to_counts(out[2]["counts"]).tolist() == [0, 1, 2, 1, 2] and string_to_counts(out[1]["counts"]).tolist() == [4, 2]
    assert rle_area(out[2]) == 2 and rle_area(out[1]) == 2 and rle_area({"size": [2, 3], "counts": [4, 2]}) == 2
    lab = np.array([[2, 0, 1], [0, 2, 1]], np.int32)
    ref = R.runs_image(lab, 6)
    assert ref[0].tolist() == runs[0].tolist() and ref[1].tolist() == [4, 4]
    assert rles_from_runs(torch.from_numpy(runs), torch.from_numpy(counts), 2, 3) == [out]
    assert rles_from_runs(np.zeros((1, 4, 2), np.int32), np.array([[1, 1]], np.int32), 2, 3) == [{}]      # all background
    with pytest.raises(ValueError, match="holds 9 runs and 4 were written"):
        rles_from_runs(runs, np.array([[9, 4]], np.int32), 2, 3)
    for seed in range(4):                                              # and every id of a block map, against the restatement
        lab = _blocks(9, 11, 4, seed, 2).astype(np.int32)
        r, c = R.runs_image(lab, 128)
        got, = rles_from_runs(r[None], c[None], 9, 11)
        want = R.label_counts(lab)
        assert list(got) == sorted(want) and all(string_to_counts(got[i]["counts"]).tolist() == want[i].tolist() for i in want)


def test_argument_errors_by_name_and_no_cpu_path():
    from camouflage_multimodal_amd import counts_to_string, decode_rles, encode_instances, label_runs, rle_area, string_to_counts
    from camouflage_multimodal_amd._lib import CamoError
    a = torch.zeros(2, 4, 4, dtype=torch.int32)
    for fn in (label_runs, encode_instances):
        for kw, word in (({"max_runs": 0}, "max_runs"), ({"max_runs": 2.5}, "max_runs"), ({"max_runs": True}, "max_runs"), ({"max_runs": 1 << 26}, "rows")):
            with pytest.raises(ValueError, match=word):
                fn(a, **kw)
        with pytest.raises(ValueError, match="labels must be int32"):
            fn(a.long())
        with pytest.raises(ValueError, match=r"need labels \[N, H, W\]"):
            fn(a[None])
        with pytest.raises(ValueError, match="labels must be a tensor"):
            fn(a.numpy())
        with pytest.raises(CamoError, match="labels is on cpu"):       # good arguments, CPU tensors: no fallback
            fn(a)
    ok = {"size": [4, 4], "counts": "4<"}                              # [4, 12]
    assert string_to_counts("4<").tolist() == [4, 12]
    for rles, word in ((None, "per_image_rles"), ([], "per_image_rles"), ([5], "image 0: need a list"), ([[5]], "image 0, annotation 0 must be a dict"),
                       ([[ok], [{"size": [4, 5], "counts": "4<"}]], r"image 1, annotation 0: size \[4, 5\]"),
                       ([[ok, {"size": [4, 4], "counts": "4;"}]], "image 0, annotation 1: the counts sum to 15"),
                       ([[{"size": [4, 4], "counts": "4="}]], "the counts sum to 17"), ([[{"size": [4, 4], "counts": "4\x7f"}]], "alphabet"),
                       ([[{"size": [4, 4], "counts": "4l"}]], "ends inside a count"), ([[{"size": [4], "counts": "4<"}]], '"size" must be'),
                       ([[{"size": [4, 4], "counts": [4, -1, 13]}]], "negative"), ([[{"size": [4, 4], "counts": [4.0, 12.0]}]], "integers"),
                       ([[(ok, 0)]], "value must be"), ([[(ok, True)]], "value must be"), ([[(ok, 2 ** 31)]], "value must be")):
        with pytest.raises(ValueError, match=word):
            decode_rles(rles, 4, 4, "cpu")
    for H, W in ((0, 4), (4, -1), (4.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="must be an integer >= 1"):
            decode_rles([[ok]], H, W, "cpu")
    for good in ([[ok]], [[(ok, 9)], []], [{3: ok}], [[]]):
        with pytest.raises(CamoError, match="no CPU fallback"):
            decode_rles(good, 4, 4, "cpu")
    with pytest.raises(ValueError, match="counts must be >= 0"):
        counts_to_string([3, -1])
    with pytest.raises(ValueError, match="integers"):
        counts_to_string([[1, 2]])
    with pytest.raises(ValueError, match="must be a string"):
        string_to_counts(5)
    with pytest.raises(ValueError, match="must be a dict"):
        rle_area("4<")


def test_pipeline_argument_errors_by_name(tmp_path):
    """``ValueError`` before anything touches the device: the model and the images stay on the CPU."""
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage, detect_camouflage_batch, detect_camouflage_directory, detect_camouflage_ragged
    m = RegionGraphGNN(hidden_channels=32, num_classes=2, heads=2).eval()
    img, gt = torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, dtype=torch.uint8)
    ragged = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="rle needs instances=True"):
        detect_camouflage_batch(m, img, device="cpu", rle=True)
    with pytest.raises(ValueError, match="rle needs instances=True"):
        detect_camouflage(m, img[0], device="cpu", rle=True)
    with pytest.raises(ValueError, match="rle needs instances=True"):
        detect_camouflage_ragged(m, ragged, device="cpu", rle=True)
    with pytest.raises(ValueError, match="rle must be True or False"):
        detect_camouflage_batch(m, img, device="cpu", instances=True, rle="coco")
    with pytest.raises(ValueError, match='"gt_labels" or "gt_rles", not both'):
        detect_camouflage_batch(m, img, device="cpu", instances=True, match={"gt_labels": torch.zeros(1, 16, 16, dtype=torch.int32), "gt_rles": [[]]})
    with pytest.raises(ValueError, match=r'match\["gt_rles"\] must be a non-empty list'):
        detect_camouflage_batch(m, img, device="cpu", instances=True, match={"gt_rles": "4<"})
    with pytest.raises(ValueError, match="results_json needs instances=True"):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", results_json=str(tmp_path / "r.json"))
    with pytest.raises(ValueError, match="image_ids needs results_json"):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", instances=True, image_ids={"a": 1})
    with pytest.raises(ValueError, match="image_ids must be a dict"):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", instances=True, results_json=str(tmp_path / "r.json"), image_ids=[1])
    with pytest.raises(ValueError, match="results_json must be a path"):
        detect_camouflage_directory(m, str(tmp_path), device="cpu", instances=True, results_json=5)
    with pytest.raises(TypeError):
        detect_camouflage_batch(m, img, gt, 500, 0.5, "cpu", False, True, 0, False, 8, None, None, True)      # rle is keyword-only


def test_header_constants_and_symbols():
    import os
    import re
    from camouflage_multimodal_amd import _lib
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "camo_rle.h")).read(), flags=re.S)
    m = dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    assert m["CAMO_RLE_MAX_ROWS"] == "(1 << 26)" and _lib.RLE_MAX_ROWS == 1 << 26 and m["CAMO_RLE_MAX_COUNTS"] == "(1 << 26)" and _lib.RLE_MAX_COUNTS == 1 << 26
    assert int(m["CAMO_RLE_MAX_ANNOTATIONS"]) == _lib.RLE_MAX_ANNOTATIONS == 65535 and _lib.ABI_VERSION == 13
    assert _lib.symbols("camo_rle.h") == ("camo_rle_runs_workspace_bytes", "camo_rle_runs", "camo_rle_decode_workspace_bytes", "camo_rle_decode")


def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced, and no device is needed."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    ws = L.camo_rle_runs_workspace_bytes
    assert ws(1, 1, 1, 1) > 0 and ws(1, 1, 1, 1) % 256 == 0 and ws(2, 65, 129, 8) > ws(1, 65, 129, 8) and ws(1, 65, 129, 8) >= 2 * 4 * 129 * 2
    assert ws(16, 256, 256, 1 << 22) > 0 and ws(1, 8, 8, 1 << 26) > 0
    for bad in ((0, 8, 8, 4), (65536, 1, 1, 1), (1, 0, 8, 4), (1, 8, -1, 4), (1, 8192, 8193, 4), (17, 8192, 8192, 4), (1, 8, 8, 0), (1, 8, 8, -2),
                (1, 8, 8, (1 << 26) + 1), (2, 8, 8, (1 << 25) + 1)):
        assert ws(*bad) == 0, bad
    wd = L.camo_rle_decode_workspace_bytes
    assert wd(1, 1, 1, 1, 0) > 0 and wd(1, 1, 1, 1, 0) % 256 == 0 and wd(3, 8, 8, 300, 5000) >= 4 * 5000 and wd(1, 8, 8, 65535, 1 << 26) > 0
    for bad in ((0, 8, 8, 1, 4), (65536, 1, 1, 1, 4), (1, 0, 8, 1, 4), (1, 8, -1, 1, 4), (1, 8192, 8193, 1, 4), (1, 8, 8, 0, 4), (1, 8, 8, 65536, 4),
                (1, 8, 8, 1, -1), (1, 8, 8, 1, (1 << 26) + 1)):
        assert wd(*bad) == 0, bad
    p, big = ctypes.c_void_p(0x1000), 1 << 40
    good = dict(labels=p, N=2, H=8, W=8, R=16, runs=p, counts=p, ws=p, nbytes=big)

    def runs(**kw):
        a = dict(good, **kw)
        return L.camo_rle_runs(a["labels"], a["N"], a["H"], a["W"], a["R"], a["runs"], a["counts"], a["ws"], a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=8192, W=8193), dict(R=0), dict(R=-1), dict(R=(1 << 25) + 1), dict(labels=None),
               dict(runs=None), dict(counts=None), dict(ws=None), dict(ws=ctypes.c_void_p(0x1080)), dict(runs=ctypes.c_void_p(0x1004)),
               dict(labels=ctypes.c_void_p(0x1002)), dict(nbytes=ws(2, 8, 8, 16) - 1), dict(nbytes=0)):
        assert runs(**kw) == -1, kw                                    # CAMO_E_ARG
        assert L.camo_last_error()
    good = dict(cnts=p, total=12, off=p, img=p, val=p, A=3, N=2, H=8, W=8, labels=p, sums=p, ws=p, nbytes=big)

    def decode(**kw):
        a = dict(good, **kw)
        return L.camo_rle_decode(a["cnts"], a["total"], a["off"], a["img"], a["val"], a["A"], a["N"], a["H"], a["W"], a["labels"], a["sums"], a["ws"],
                                 a["nbytes"], None)
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=8192, W=8193), dict(A=0), dict(A=65536), dict(total=-1), dict(total=(1 << 26) + 1),
               dict(cnts=None), dict(off=None), dict(img=None), dict(val=None), dict(labels=None), dict(sums=None), dict(ws=None),
               dict(sums=ctypes.c_void_p(0x1004)), dict(ws=ctypes.c_void_p(0x1080)), dict(nbytes=wd(2, 8, 8, 3, 12) - 1), dict(nbytes=0)):
        assert decode(**kw) == -1, kw
        assert L.camo_last_error()


# ---- GPU: the kernels against the restatement, byte for byte ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_runs_equal_the_restatement_bytewise(name):
    labels, R_ = _case(name)
    got, want = _raw_runs(labels, R_), R.runs_batch(labels, R_)
    _same(got, want, name)
    if name == "checkerboard":
        assert got["counts"].tolist() == [[65 * 129, 65 * 129]] and (got["runs"][0, :, 0] == np.arange(65 * 129)).all()
    if name == "checkerboard_short":
        assert got["counts"].tolist() == [[65 * 129, 65 * 129 - 1]]      # the guard behind runs holds what the last run would have overwritten
    if name == "crossing":
        assert got["counts"][0, 0] == 6 and got["runs"][0, 1].tolist() == [4 * 70 + 60, 3] and got["runs"][0, 2].tolist() == [5 * 70 + 5, 0]
    if name.startswith(("background", "one_id")):
        assert got["counts"].tolist() == [[1, 1]] and got["runs"][0, 0].tolist() == [0, 0 if name.startswith("background") else 7]


@pytest.mark.gpu
def test_runs_of_a_capacity_of_one_and_of_a_far_larger_one():
    labels, _ = _case("blocks@65x129")
    for R_ in (1, 2, 20000):
        _same(_raw_runs(labels, R_), R.runs_batch(labels, R_), R_)


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_are_the_same_bytes():
    labels, R_ = _case("batch")
    whole, again = _raw_runs(labels, R_), _raw_runs(labels, R_)
    _same(again, whole, "second call")
    for n in range(len(labels)):
        _same(_raw_runs(labels[n:n + 1], R_), {k: whole[k][n:n + 1] for k in whole}, f"image {n}")


def _blob_maps():
    rng = np.random.default_rng(30)
    y, x = np.mgrid[0:70, 0:33]
    prob = np.zeros((2, 70, 33), np.float32)
    for n in range(2):
        for cy, cx, r in zip(rng.integers(4, 66, 7), rng.integers(4, 29, 7), rng.integers(2, 7, 7)):
            prob[n] = np.maximum(prob[n], np.where((y - cy) ** 2 + (x - cx) ** 2 <= r * r, rng.uniform(0.55, 1.0), 0.0).astype(np.float32))
    return prob


@pytest.mark.gpu
def test_runs_and_rles_of_real_instances():
    from camouflage_multimodal_amd import decode_rles, encode_instances, label_runs, mask_instances, rle_area, rles_from_runs, string_to_counts
    found = mask_instances(torch.from_numpy(_blob_maps()).cuda(), max_instances=16)
    labels = found["labels"].cpu().numpy()
    assert labels.max() >= 3
    out = label_runs(found["labels"], 512)
    _same({k: out[k].cpu().numpy() for k in out}, R.runs_batch(labels, 512), "label_runs")
    _same(_raw_runs(labels, 512), R.runs_batch(labels, 512), "raw")
    rles = rles_from_runs(out["runs"], out["counts"], 70, 33)
    assert rles == encode_instances(found["labels"]) == encode_instances(found["labels"], max_runs=2)      # the second call holds every run
    table = found["table"].cpu().numpy()
    for n in range(2):
        want = R.label_counts(labels[n])
        assert list(rles[n]) == sorted(want)
        for i, c in want.items():
            assert rles[n][i]["size"] == [70, 33] and string_to_counts(rles[n][i]["counts"]).tolist() == c.tolist() and rle_area(rles[n][i]) == table[n, i - 1, 0]
    back = decode_rles(rles, 70, 33)
    assert back.dtype == torch.int32 and torch.equal(back, found["labels"])
    one = encode_instances(found["labels"][0])                          # [H, W]
    assert one == rles[:1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_decode_of_encode_is_the_label_map(name):
    from camouflage_multimodal_amd import decode_rles, encode_instances
    labels, _ = _case(name)
    N, H, W = labels.shape
    lab = torch.from_numpy(labels).cuda()
    rles = encode_instances(lab, max_runs=64)
    assert [sorted(r) for r in rles] == [np.unique(l[l > 0]).tolist() for l in labels]
    back = decode_rles(rles, H, W)
    assert back.cpu().numpy().tobytes() == np.where(labels > 0, labels, 0).astype(np.int32).tobytes()


@pytest.mark.gpu
def test_decode_hand_cases_overlap_short_long_and_invalid():
    H, W, HW = 7, 5, 35
    # image 0: two overlapping annotations, the larger value first and then last; a leading zero count; no foreground at all
    per_image = [[([3, 10, 22], 5), ([8, 10, 17], 2), ([0, 4, 31], 1), ([35], 9), ([8, 10, 17], 7)],
                 [([34, 1], 3), ([0, 35], 1)],
                 [([5, 5, 5, 5, 5, 5, 4], 4), ([5, 5, 5, 5, 5, 5, 6], 6), ([30, 50], 8), ([40, 3], 9), ([35, 3], 9)]]      # one short, one long, past the end
    arrays = _annotation_arrays(per_image)
    got, want = _raw_decode(*arrays, 3, H, W), R.decode(*arrays, 3, H, W)
    _same(got, dict(zip(("labels", "ann_sum"), want)), "hand cases")
    assert got["ann_sum"].tolist() == [35, 35, 35, 35, 35, 35, 35, 34, 36, 80, 43, 38]
    flat = got["labels"][0].flatten(order="F")
    assert flat[:3].tolist() == [1, 1, 1] and flat[3] == 5 and (flat[4:8] == 5).all() and (flat[8:18] == 7).all() and not flat[18:].any()
    assert got["labels"][1].flatten(order="F").tolist() == [1] * 34 + [3]
    swapped = [list(reversed(anns)) for anns in per_image]             # the largest value wins whichever comes first
    _same(_raw_decode(*_annotation_arrays(swapped), 3, H, W), {"labels": want[0]}, "reversed lists", ("labels",))
    # invalid annotations write nothing and get -1; the valid one beside them is painted
    cnts, off, img, val = _annotation_arrays([[([1, -1, 35], 4), ([2, 3, 30], 0), ([2, 3, 30], -5), ([4, 2, 29], 2)], []])
    img += [2, -1]; val += [3, 3]; cnts += [0, 35, 0, 35]; off += [off[-1] + 2, off[-1] + 4]      # images outside 0 .. N - 1
    got, want = _raw_decode(cnts, off, img, val, 2, H, W), R.decode(cnts, off, img, val, 2, H, W)
    _same(got, dict(zip(("labels", "ann_sum"), want)), "invalid")
    assert got["ann_sum"].tolist() == [-1, -1, -1, 35, -1, -1] and got["labels"].sum() == 4 and not got["labels"][1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 300])
def test_decode_of_many_annotations_over_three_images(A):
    from camouflage_multimodal_amd.rle import decode_counts
    rng = np.random.default_rng(A)
    H, W, N = 33, 70, 3
    per_image = [[] for _ in range(N)]
    for a in range(A):
        mask = np.zeros((H, W), bool)
        y0, x0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
        mask[y0:y0 + int(rng.integers(1, 12)), x0:x0 + int(rng.integers(1, 12))] = a % 17 != 5      # (some annotations are empty)
        per_image[int(rng.integers(0, N))].append((R.mask_counts(mask), int(rng.integers(1, 40))))
    arrays = _annotation_arrays(per_image)
    got, want = _raw_decode(*arrays, N, H, W), R.decode(*arrays, N, H, W)
    _same(got, dict(zip(("labels", "ann_sum"), want)), A)
    assert (got["ann_sum"] == H * W).all() and got["labels"].any()
    labels, sums = decode_counts(*arrays, N, H, W)
    assert labels.cpu().numpy().tobytes() == want[0].tobytes() and sums.cpu().numpy().tobytes() == want[1].tobytes()


@pytest.mark.gpu
def test_decode_rles_values_and_forms():
    from camouflage_multimodal_amd import counts_to_string, decode_rles
    H, W = 7, 5
    a = {"size": [H, W], "counts": counts_to_string([3, 10, 22])}
    b = {"size": [H, W], "counts": [8, 10, 17]}                          # an uncompressed RLE: the counts as a list
    later = decode_rles([[a, b], []], H, W)                              # values 1, 2 in list order: the later one wins
    flat = later[0].cpu().numpy().flatten(order="F")
    assert later.shape == (2, H, W) and flat.tolist() == [0] * 3 + [1] * 5 + [2] * 10 + [0] * 17 and not later[1].any()
    assert decode_rles([[(a, 9), (b, 4)], []], H, W)[0].cpu().numpy().flatten(order="F").tolist() == [0] * 3 + [9] * 10 + [4] * 5 + [0] * 17
    assert torch.equal(decode_rles([{9: a, 4: b}, {}], H, W), decode_rles([[(a, 9), (b, 4)], []], H, W))
    none = decode_rles([[], []], H, W)
    assert none.shape == (2, H, W) and none.dtype == torch.int32 and none.is_cuda and not none.any()
