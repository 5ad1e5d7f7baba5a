"""Instance matching (include/camo_inst_match.h): the numpy restatement tests/inst_match_ref.py against brute force and
hand cases (CPU, no library call), and the kernels against the restatement byte for byte (GPU).

The GPU cases give the label maps directly as int32 tensors, so the kernels meet what camo_instances would rarely produce: pairs
that change at every pixel, ids past the tables, 300 ids in use.  Every raw call places its six outputs between guard bytes."""
import ctypes
import functools
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest
import torch

import inst_match_ref as R
from conftest import ROOT
from inst_match_ref import blocks as _blocks, score_table as _table
from raw_calls import BUILDERS, MATCH_NAMES as NAMES, execute, same_bytes as _same

STRIP10 = (np.array([[1, 1, 1, 1, 2, 2, 2, 2, 2, 2]]), np.array([[0, 0, 1, 1, 1, 1, 1, 1, 2, 2]]))
STRIP4 = (np.array([[1, 1, 1, 1]]), np.array([[1, 1, 2, 2]]))


def _row(area, sq):
    return [area, 0, 0, 0, 0, 0, 0, sq]


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (pred [N, H, W], gt [N, H, W], P, G, table [N, rows, 8] or None, thresholds)"""
    table, thr = None, R.COCO
    if name in ("strip10", "strip10_swapped"):
        pred, gt, P, G, thr = STRIP10[0][None], STRIP10[1][None], 2, 2, (F(1, 4), F(1, 2))
        if name == "strip10_swapped":
            table = np.array([[_row(4, 100), _row(6, 900)]], np.int64)
    elif name == "strip4":
        pred, gt, P, G, thr = STRIP4[0][None], STRIP4[1][None], 1, 2, (F(10, 20), F(11, 20))
    elif name == "narrow_7x5":
        pred, gt, P, G = _blocks(7, 5, 3, 1, 3)[None], np.roll(_blocks(7, 5, 3, 2, 3), 1, 1)[None], 3, 3
    elif name == "odd_33x31":
        pred, gt, P, G, table = _blocks(33, 31, 9, 3)[None], np.roll(_blocks(33, 31, 9, 3), 1, 1)[None], 9, 9, _table(1, 9, 4)
    elif name == "one_pair":
        pred, gt, P, G = np.ones((1, 64, 64), np.int64), np.ones((1, 64, 64), np.int64), 4, 3
    elif name == "pairs_40x37":
        y, x = np.mgrid[0:64, 0:64]
        pred, gt, P, G, table = ((x + y) % 40 + 1)[None], ((x * 3 + y) % 37 + 1)[None], 40, 37, _table(1, 40, 5)
    elif name == "ids_300":
        idx = np.arange(1600).reshape(40, 40)
        pred, gt, P, G, table, thr = ((idx // 5) % 300 + 1)[None], (((idx + 1) // 5) % 300 + 1)[None], 300, 300, _table(1, 300, 6), (F(1, 2), F(13, 20), F(3, 4))
    elif name == "background_pred":
        pred, gt, P, G = np.zeros((1, 20, 24), np.int64), _blocks(20, 24, 4, 7)[None], 4, 4
    elif name == "background_gt":
        pred, gt, P, G, table = _blocks(20, 24, 4, 8)[None], np.zeros((1, 20, 24), np.int64), 4, 4, _table(1, 4, 9)
    elif name == "one_id":
        pred, gt, P, G = (_blocks(16, 16, 1, 10) > 0)[None].astype(np.int64), (_blocks(16, 16, 1, 11) > 0)[None].astype(np.int64), 1, 1
    elif name == "out_of_range":
        pred, gt, P, G = _blocks(24, 40, 5, 12)[None].copy(), np.roll(_blocks(24, 40, 5, 12), 2, 0)[None].copy(), 5, 5
        pred[0, 0, :7], pred[0, 3, 4:9], gt[0, 5, :11], gt[0, 0, 2:5] = -1, P + 1, G + 7, -1      # (pixel (0, 2 .. 4): both out of range)
    elif name == "score_fallback":
        pred, gt, P, G = _blocks(32, 32, 8, 13)[None], np.roll(_blocks(32, 32, 8, 13), 1, 0)[None], 8, 8
        # ids 1 and 2 tie (2 / 1 = 20 / 10), 3 has area 0, 4 has Sq > 255 area, 5 a negative Sq, 6 an area past the limit: all four score 0
        table = np.array([[_row(5, 10), _row(10, 20), _row(0, 7), _row(2, 511), _row(3, -1), _row((1 << 26) + 1, 5), _row(4, 1020), _row(7, 3)]], np.int64)
    elif name == "short_table":
        pred, gt, P, G, table = _blocks(32, 32, 8, 14)[None], np.roll(_blocks(32, 32, 8, 14), 1, 1)[None], 8, 8, _table(1, 3, 15)
    elif name == "one_threshold":
        pred, gt, P, G, thr = _blocks(32, 32, 6, 16)[None], np.roll(_blocks(32, 32, 6, 16), 1, 1)[None], 6, 6, (F(7, 10),)
    elif name == "sixteen_thresholds":
        pred, gt, P, G, table = _blocks(32, 32, 6, 17)[None], np.roll(_blocks(32, 32, 6, 17), 1, 1)[None], 6, 6, _table(1, 6, 18)
        thr = tuple(F(n, 32) for n in range(2, 33, 2))
    elif name == "batch":
        pred = np.stack([_blocks(37, 29, 7, 20 + n, 5) for n in range(5)])
        gt = np.stack([np.roll(_blocks(37, 29, 7, 20 + n, 5), n % 3, n % 2) for n in range(5)])
        P, G, table = 7, 7, _table(5, 7, 19)
    else:
        raise KeyError(name)
    return pred.astype(np.int32), gt.astype(np.int32), P, G, table, thr


CASES = ["strip10", "strip10_swapped", "strip4", "narrow_7x5", "odd_33x31", "one_pair", "pairs_40x37", "ids_300", "background_pred", "background_gt",
         "one_id", "out_of_range", "score_fallback", "short_table", "one_threshold", "sixteen_thresholds", "batch"]


@functools.lru_cache(maxsize=None)
def _ref(name):
    pred, gt, P, G, table, thr = _case(name)
    return R.match_batch(pred, gt, P, G, table, thr)


def _raw(pred, gt, P, G, table, thr):
    """camo_inst_match on guarded buffers (tests/raw_calls.py): the six outputs start from 0xA5 (the restatement holds -1 entries, which
    0xFF would let a missed store pass) and are 4-byte aligned and no more, the workspace from 0xFF -> the outputs as numpy arrays."""
    return execute(BUILDERS["camo_inst_match"](pred, gt, P, G, table, thr), 0xA5, ws_fill=0xFF, skew=4)


# ---- CPU: the restatement itself, no library call ---------------------------------------------------------------------------

def test_restated_overlap_equals_brute_force():
    rng = np.random.default_rng(0)
    for trial in range(4):
        P, G = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        pred, gt = rng.integers(-1, P + 3, (9, 11)), rng.integers(-1, G + 3, (9, 11))
        inter, oob_p, oob_g = R.overlap(pred, gt, P, G)
        for a in range(P + 1):
            for b in range(G + 1):
                assert inter[a, b] == ((pred == a) & (gt == b)).sum()
        assert oob_p == ((pred < 0) | (pred > P)).sum() and oob_g == ((gt < 0) | (gt > G)).sum()
        out = R.match_image(pred, gt, P, G)
        assert (out["pred_rows"][:, 0] == out["inter"].sum(axis=1)[1:]).all() and (out["gt_area"] == out["inter"].sum(axis=0)[1:]).all()


def test_above_one_half_the_match_is_forced():
    """Predicted ids are disjoint and so are ground-truth ids: above 1/2 at most one pair per row and per column has IoU >= t, and the
    greedy match, whatever the order, is exactly that set."""
    rng = np.random.default_rng(1)
    thr = (F(11, 20), F(3, 5), F(3, 4), F(9, 10), F(1, 1))
    for trial in range(300):
        P, G = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        pred = _blocks(8, 8, P, 1000 + trial, int(rng.integers(2, 5)))
        gt = np.roll(_blocks(8, 8, G, 1000 + trial if trial % 2 else 5000 + trial, int(rng.integers(2, 5))), int(rng.integers(0, 2)), 1)
        table = _table(1, P, trial)[0] if trial % 3 else None
        out = R.match_image(pred, gt, P, G, table, thr)
        inter = out["inter"].astype(np.int64)
        ap, ag = inter.sum(axis=1), inter.sum(axis=0)
        for k, t in enumerate(thr):
            forced = {(p, g) for p in range(1, P + 1) for g in range(1, G + 1)
                      if inter[p, g] and F(int(inter[p, g]), int(ap[p] + ag[g] - inter[p, g])) >= t}
            assert forced == {(p + 1, int(g)) for p, g in enumerate(out["match"][k]) if g}, (trial, k)
            assert forced == {(int(p), g + 1) for g, p in enumerate(out["gt_match"][k]) if p}, (trial, k)


def test_hand_cases_of_the_greedy_match():
    pred, gt = STRIP10
    first = R.match_image(pred, gt, 2, 2, None, (F(1, 4), F(1, 2)))
    assert first["inter"].tolist() == [[0, 0, 0], [2, 2, 0], [0, 4, 2]]
    assert first["match"].tolist() == [[1, 2], [0, 1]] and first["gt_match"].tolist() == [[1, 2], [2, 0]]
    assert first["pred_rows"].tolist() == [[4, 0, 1, 2], [6, 1, 1, 4]] and first["gt_area"].tolist() == [6, 2] and first["counts"].tolist() == [0, 0, 2, 2]
    swapped = R.match_image(pred, gt, 2, 2, [_row(4, 100), _row(6, 900)], (F(1, 4), F(1, 2)))
    assert swapped["match"].tolist() == [[0, 1], [0, 1]]              # greedy is not the per-row argmax: id 2 took ground truth 1 first
    assert swapped["pred_rows"][:, 1].tolist() == [1, 0]
    pred, gt = STRIP4
    half = R.match_image(pred, gt, 1, 2, None, (F(10, 20), F(11, 20)))
    assert half["match"].tolist() == [[1], [0]] and half["pred_rows"].tolist() == [[4, 0, 1, 2]]      # both IoUs are 1/2: the smaller id


def test_average_precision_hand_cases():
    from camouflage_multimodal_amd.instance_match import InstanceAP, average_precision
    for ap in (R.average_precision, average_precision):
        assert ap([(0.9, False), (0.8, True)], 1) == pytest.approx(0.5, abs=1e-12)
        assert ap([(0.9, True), (0.8, False), (0.7, True)], 2) == pytest.approx((51 + 50 * 2 / 3) / 101, abs=1e-12)
        assert ap([(0.9, True), (0.8, True)], 2) == pytest.approx(1.0, abs=1e-12)
        assert ap([(0.5, True), (0.5, False)], 1) == pytest.approx(1.0, abs=1e-12)      # equal scores: insertion order
        assert ap([(0.9, False)], 0) is None and ap([], 3) == 0.0
    half = (F(1, 2), F(3, 4))
    rec = [{"thresholds": half, "n_pred": 3, "n_gt": 2,
            "predictions": [{"id": 1, "matches": [1, 1]}, {"id": 2, "matches": [0, 0]}, {"id": 3, "matches": [2, 0]}]}]
    res = InstanceAP().add(rec, [[0.9, 0.8, 0.7]]).result()
    assert res["AP50"] == pytest.approx((51 + 50 * 2 / 3) / 101) and res["AP75"] == pytest.approx(51 / 101) and res["AP"] == pytest.approx((res["AP50"] + res["AP75"]) / 2)
    assert res["AR"] == pytest.approx(0.75) and res["n_gt"] == 2 and res["n_pred"] == 3
    none = InstanceAP().add([{"thresholds": half, "n_pred": 1, "n_gt": 0, "predictions": [{"id": 1, "matches": [0, 0]}]}], [[0.5]]).result()
    assert none["AP"] is None and InstanceAP().result()["AP"] is None
    with pytest.raises(ValueError, match="different thresholds"):
        InstanceAP().add(rec, [[0.9, 0.8, 0.7]]).add([dict(rec[0], thresholds=(F(1, 2),))], [[0.9, 0.8, 0.7]])
    with pytest.raises(ValueError, match="no score for predicted id 3"):
        InstanceAP().add(rec, [[0.9, 0.8]])


def test_header_constants_and_abi_version():
    from camouflage_multimodal_amd import _lib

    def macros(header):
        text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return dict(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(CAMO_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M))
    m = macros("camo_inst_match.h")
    assert int(m["CAMO_IM_MAX_THRESHOLDS"]) == _lib.IM_MAX_THRESHOLDS == 16 and int(m["CAMO_IM_MAX_IDS"]) == _lib.IM_MAX_IDS == 1024
    assert m["CAMO_IM_MAX_CELLS"] == "(1 << 26)" and _lib.IM_MAX_CELLS == 1 << 26 and int(m["CAMO_IM_COUNTS"]) == _lib.IM_COUNTS == 4
    assert int(macros("camo_fusion.h")["CAMO_ABI_VERSION"]) == _lib.ABI_VERSION == 13
    assert int(macros("camo_rg_detect.h")["CAMO_RGD_MAX_IMAGE_PIXELS"].strip("()").split("<<")[1]) == 26 and R.MAX_IMAGE_PIXELS == 1 << 26
    assert _lib.symbols("camo_inst_match.h") == ("camo_inst_match_workspace_bytes", "camo_inst_match")


def test_argument_errors_by_name_and_no_cpu_path():
    from camouflage_multimodal_amd import match_instances
    from camouflage_multimodal_amd._lib import CamoError
    from camouflage_multimodal_amd.instance_match import match_thresholds
    a = torch.zeros(2, 4, 4, dtype=torch.int32)
    tab = torch.zeros(2, 3, 8, dtype=torch.int64)
    for kw, word in (({"max_pred": 0}, "max_pred"), ({"max_pred": 1025}, "max_pred"), ({"max_pred": 2.5}, "max_pred"), ({"max_pred": True}, "max_pred"),
                     ({"max_gt": 0}, "max_gt"), ({"max_gt": 1025}, "max_gt"), ({"max_gt": "4"}, "max_gt"),
                     ({"thresholds": ()}, "thresholds"), ({"thresholds": [F(1, 2)] * 17}, "thresholds"), ({"thresholds": 0.5}, "thresholds"),
                     ({"thresholds": [0.0]}, "thresholds"), ({"thresholds": [1.5]}, "thresholds"), ({"thresholds": [0.12345]}, "thresholds"),
                     ({"thresholds": [F(1, 1001)]}, "thresholds"), ({"thresholds": [F(1, 7), F(1, 11), F(1, 13), F(1, 2)]}, "denominator"),
                     ({"thresholds": [(1, 0)]}, "thresholds"), ({"thresholds": ["0.5"]}, "thresholds"), ({"thresholds": [True]}, "thresholds"),
                     ({"thresholds": [float("nan")]}, "thresholds"), ({"thresholds": [(-1, 2)]}, "thresholds"),
                     ({"pred_table": torch.zeros(2, 3, 7, dtype=torch.int64)}, "pred_table"), ({"pred_table": torch.zeros(3, 3, 8, dtype=torch.int64)}, "pred_table"),
                     ({"pred_table": torch.zeros(2, 3, 8)}, "pred_table"), ({"pred_table": torch.zeros(2, 0, 8, dtype=torch.int64)}, "pred_table")):
        with pytest.raises(ValueError, match=word):
            match_instances(a, a, **kw)
    with pytest.raises(ValueError, match="table cells"):
        match_instances(torch.zeros(64, 2, 2, dtype=torch.int32), torch.zeros(64, 2, 2, dtype=torch.int32), max_pred=1024, max_gt=1024)
    with pytest.raises(ValueError, match="pred_labels must be int32"):
        match_instances(a.long(), a)
    with pytest.raises(ValueError, match="gt_labels must be int32"):
        match_instances(a, a.float())
    with pytest.raises(ValueError, match="gt_labels of pred_labels' shape"):
        match_instances(a, a[:1])
    with pytest.raises(ValueError, match=r"need pred_labels \[N, H, W\]"):
        match_instances(a[None], a[None])
    with pytest.raises(ValueError, match="must be tensors"):
        match_instances(a.numpy(), a)
    for kw in ({}, {"pred_table": tab}, {"max_pred": 5, "max_gt": 1024, "thresholds": [0.5, (3, 4), F(9, 10)]}):
        with pytest.raises(CamoError, match="pred_labels is on cpu"):      # good arguments, CPU tensors: no fallback
            match_instances(a, a, **kw)
    fr, nums, den = match_thresholds([0.5, (3, 4), F(9, 10), 0.125, 1])
    assert fr == (F(1, 2), F(3, 4), F(9, 10), F(1, 8), F(1)) and den == 40 and nums == [20, 30, 36, 5, 40]
    assert match_thresholds()[1:] == (list(range(10, 20)), 20)


def test_records_arithmetic_from_the_integers():
    """instance_match_records on the restatement's integers (CPU tensors: the copy is a no-op)."""
    from camouflage_multimodal_amd import instance_match_records
    pred, gt = STRIP10
    out = {k: torch.from_numpy(v[None]) for k, v in R.match_image(pred, gt, 2, 2, None, (F(1, 4), F(1, 2))).items()}
    out["thresholds"] = (F(1, 4), F(1, 2))
    rec, = instance_match_records(out)
    assert rec["per_threshold"][0] == {"tp": 2, "fp": 0, "fn": 0, "precision": 1.0, "recall": 1.0, "f1": 1.0}
    assert rec["per_threshold"][1] == {"tp": 1, "fp": 1, "fn": 1, "precision": 0.5, "recall": 0.5, "f1": 0.5}
    assert rec["predictions"] == [{"id": 1, "area": 4, "rank": 0, "best_gt": 1, "best_iou": 0.25, "matches": [1, 0]},
                                  {"id": 2, "area": 6, "rank": 1, "best_gt": 1, "best_iou": 0.5, "matches": [2, 1]}]
    # at 1/2 the pair (2, 1) has IoU exactly 1/2: not 2 i > u, so no pair enters the panoptic quality
    assert (rec["pq"], rec["sq"], rec["rq"]) == (0.0, 0.0, 0.0) and rec["n_pred"] == rec["n_gt"] == 2 and not rec["truncated_pred"] and not rec["truncated_gt"]
    p2, g2 = np.array([[1, 1, 1, 1, 0, 2, 2, 2, 9]]), np.array([[1, 1, 1, 0, 0, 0, 0, 2, 2]])
    out = {k: torch.from_numpy(v[None]) for k, v in R.match_image(p2, g2, 2, 2, None, (F(1, 2),)).items()}
    out["thresholds"] = (F(1, 2),)
    rec, = instance_match_records(out)
    assert rec["truncated_pred"] and not rec["truncated_gt"] and rec["per_threshold"][0]["tp"] == 1      # (3/4; 1/3 is below 1/2)
    assert rec["sq"] == 0.75 and rec["rq"] == 0.5 and rec["pq"] == 0.375
    out["thresholds"] = (F(3, 4),)
    assert instance_match_records(out)[0]["pq"] is None


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_kernels_equal_the_restatement_bytewise(name):
    _same(_raw(*_case(name)), _ref(name), name)


@pytest.mark.gpu
def test_strips_on_the_device_are_the_hand_cases():
    first, swapped, half = _raw(*_case("strip10")), _raw(*_case("strip10_swapped")), _raw(*_case("strip4"))
    assert first["match"][0].tolist() == [[1, 2], [0, 1]] and swapped["match"][0].tolist() == [[0, 1], [0, 1]] and half["match"][0].tolist() == [[1], [0]]


@pytest.mark.gpu
def test_a_batch_is_its_images_and_two_calls_are_the_same_bytes():
    pred, gt, P, G, table, thr = _case("batch")
    whole, again = _raw(pred, gt, P, G, table, thr), _raw(pred, gt, P, G, table, thr)
    _same(again, whole, "second call")
    for n in range(len(pred)):
        one = _raw(pred[n:n + 1], gt[n:n + 1], P, G, table[n:n + 1], thr)
        _same(one, {k: whole[k][n:n + 1] for k in NAMES}, f"image {n}")


@pytest.mark.gpu
def test_match_instances_is_the_raw_call():
    from camouflage_multimodal_amd import instance_match_records, match_instances
    for name in ("pairs_40x37", "out_of_range", "batch"):
        pred, gt, P, G, table, thr = _case(name)
        out = match_instances(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), None if table is None else torch.from_numpy(table).cuda(),
                              None if table is not None else P, G, thr)
        _same({k: out[k].cpu().numpy() for k in NAMES}, _ref(name), name)
        assert out["thresholds"] == tuple(thr)
        rec = instance_match_records(out)
        want = _ref(name)
        for n, r in enumerate(rec):
            assert [p["id"] for p in r["predictions"]] == [p + 1 for p in range(P) if want["pred_rows"][n, p, 0] > 0]
            assert r["n_pred"] == want["counts"][n, 2] and r["truncated_pred"] == bool(want["counts"][n, 0])
            assert [t["tp"] for t in r["per_threshold"]] == (want["match"][n] > 0).sum(axis=1).tolist()
    one = match_instances(torch.from_numpy(STRIP4[0].astype(np.int32)).cuda(), torch.from_numpy(STRIP4[1].astype(np.int32)).cuda())      # [H, W], the defaults
    assert one["inter"].shape == (1, 65, 65) and one["match"].shape == (1, 10, 64) and one["match"][0, :, 0].tolist() == [1] + [0] * 9


@pytest.mark.gpu
def test_end_to_end_from_probability_maps():
    """mask_instances of a blob map against mask_instances of a shifted copy, held to the two restatements chained."""
    import instances_ref as IR
    from camouflage_multimodal_amd import mask_instances, match_instances
    rng = np.random.default_rng(30)
    y, x = np.mgrid[0:48, 0:56]
    prob = np.zeros((2, 48, 56), np.float32)
    for n in range(2):
        for cy, cx, r in zip(rng.integers(6, 42, 6), rng.integers(6, 50, 6), rng.integers(3, 8, 6)):
            prob[n] = np.maximum(prob[n], np.where((y - cy) ** 2 + (x - cx) ** 2 <= r * r, rng.uniform(0.55, 1.0), 0.0).astype(np.float32))
    shifted = np.roll(prob, (1, 2), (1, 2))
    dp, dg = mask_instances(torch.from_numpy(prob).cuda(), max_instances=8), mask_instances(torch.from_numpy(shifted).cuda(), max_instances=8)
    rp, rg = IR.instances(prob, max_instances=8), IR.instances(shifted, max_instances=8)
    assert (dp["labels"].cpu().numpy() == rp[0]).all() and (dg["labels"].cpu().numpy() == rg[0]).all()
    out = match_instances(dp["labels"], dg["labels"], dp["table"], max_gt=8)
    _same({k: out[k].cpu().numpy() for k in NAMES}, R.match_batch(rp[0], rg[0], 8, 8, rp[2], R.COCO), "end to end")
    assert (out["match"][:, 0] > 0).any()


@pytest.mark.gpu
def test_workspace_and_argument_checks_of_the_library():
    """Every check runs on the host before any launch: the pointers below are never dereferenced."""
    from camouflage_multimodal_amd import _lib
    L = _lib.lib()
    ws = L.camo_inst_match_workspace_bytes
    assert ws(1, 1, 1, 1, 1, 1) > 0 and ws(1, 1, 1, 1, 1, 1) % 256 == 0 and ws(2, 8, 8, 64, 64, 10) > ws(1, 8, 8, 64, 64, 10)
    assert ws(16, 256, 256, 1024, 1024, 16) > 0 and ws(63, 8, 8, 1024, 1024, 16) > 0 and ws(64, 8, 8, 1024, 1024, 16) == 0
    for bad in ((0, 8, 8, 4, 4, 1), (65536, 1, 1, 1, 1, 1), (1, 0, 8, 4, 4, 1), (1, 8, -1, 4, 4, 1), (1, 8192, 8193, 4, 4, 1), (17, 8192, 8192, 4, 4, 1),
                (1, 8, 8, 0, 4, 1), (1, 8, 8, 1025, 4, 1), (1, 8, 8, 4, 0, 1), (1, 8, 8, 4, 1025, 1), (1, 8, 8, 4, 4, 0), (1, 8, 8, 4, 4, 17)):
        assert ws(*bad) == 0, bad
    p, big = ctypes.c_void_p(0x1000), 1 << 40
    thr = (ctypes.c_int32 * 16)(*range(10, 26))
    good = dict(pl=p, gl=p, N=2, H=8, W=8, P=4, G=4, table=p, rows=4, thr=thr, den=25, T=10, inter=p, pred_rows=p, gt_area=p, match=p, gt_match=p, counts=p,
                ws=p, nbytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return L.camo_inst_match(a["pl"], a["gl"], a["N"], a["H"], a["W"], a["P"], a["G"], a["table"], a["rows"], a["thr"], a["den"], a["T"], a["inter"],
                                 a["pred_rows"], a["gt_area"], a["match"], a["gt_match"], a["counts"], a["ws"], a["nbytes"], None)
    bad = [dict(N=0), dict(N=65536), dict(H=0), dict(W=-3), dict(H=8192, W=8193), dict(P=0), dict(P=1025), dict(G=0), dict(G=1025),
           dict(N=64, P=1024, G=1024), dict(T=0), dict(T=17), dict(den=0), dict(den=1001), dict(den=18), dict(thr=None),
           dict(thr=(ctypes.c_int32 * 16)(0, *range(11, 26))), dict(thr=(ctypes.c_int32 * 16)(-5, *range(11, 26))), dict(rows=0), dict(rows=-1),
           dict(table=ctypes.c_void_p(0x1004)), dict(pl=None), dict(gl=None), dict(inter=None), dict(pred_rows=None), dict(gt_area=None), dict(match=None),
           dict(gt_match=None), dict(counts=None), dict(ws=None), dict(ws=ctypes.c_void_p(0x1080)), dict(nbytes=ws(2, 8, 8, 4, 4, 10) - 1), dict(nbytes=0)]
    for kw in bad:
        assert call(**kw) == -1, kw                                  # CAMO_E_ARG
        assert L.camo_last_error()
