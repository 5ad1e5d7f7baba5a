"""Instance matching on MI355X (include/camo_inst_match.h): are the objects a predicted mask holds the right ones?

``match_instances`` runs ``camo_inst_match`` on two label maps -- the pixels of every (predicted id, ground-truth id) pair, and the
greedy matches of predictions to ground truth in score order at each IoU threshold -- and returns device tensors;
``instance_match_records`` takes the ratios (IoU, precision, recall, F1, panoptic quality) from the integers on the host in float64;
``InstanceAP`` accumulates records over a dataset into COCO's 101-point average precision.
PARITY UNPINNED: the header's text is the definition (restated in numpy in tests/inst_match_ref.py).  There is no CPU path: tensors
that are not on a HIP device raise.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os
from fractions import Fraction
from functools import partial
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, workspace
from .instances import mask_instances

COCO = tuple(Fraction(n, 20) for n in range(10, 20))
MAX_DENOMINATOR = 1000


def match_thresholds(thresholds=COCO):
    """``thresholds`` -- ``fractions.Fraction``s, (num, den) pairs of integers, or floats equal to n / 1000 -- as (the tuple of
    Fractions, their numerators over the common denominator, that denominator); the ``ValueError`` of a bad one by name."""
    try:
        items = list(thresholds)
    except TypeError:
        raise ValueError(f"thresholds must be a sequence, got {thresholds!r}") from None
    if not 1 <= len(items) <= _lib.IM_MAX_THRESHOLDS:
        raise ValueError(f"thresholds must hold 1 .. {_lib.IM_MAX_THRESHOLDS} values, got {len(items)}")
    fr = []
    for t in items:
        if isinstance(t, bool):
            raise ValueError(f"thresholds: {t!r} is not a fraction, a (num, den) pair or a float")
        if isinstance(t, numbers.Rational):
            f = Fraction(t)
        elif isinstance(t, (tuple, list)) and len(t) == 2 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in t) and t[1] > 0:
            f = Fraction(int(t[0]), int(t[1]))
        elif isinstance(t, float) and math.isfinite(t):
            n = round(t * 1000)
            if n / 1000 != t:
                raise ValueError(f"thresholds: the float {t!r} is not n / 1000; give a Fraction or a (num, den) pair")
            f = Fraction(n, 1000)
        else:
            raise ValueError(f"thresholds: {t!r} is not a fraction, a (num, den) pair or a float")
        if not 0 < f <= 1:
            raise ValueError(f"thresholds: {t!r} is not in (0, 1]")
        fr.append(f)
    den = 1
    for f in fr:
        den = den * f.denominator // math.gcd(den, f.denominator)
    if den > MAX_DENOMINATOR:
        raise ValueError(f"thresholds: the common denominator {den} exceeds {MAX_DENOMINATOR}")
    return tuple(fr), [int(f * den) for f in fr], den


def _id_bound(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= _lib.IM_MAX_IDS:
        raise ValueError(f"{name} must be an integer in [1, {_lib.IM_MAX_IDS}], got {v!r}")
    return int(v)


def _match_inputs(pred_labels, gt_labels, pred_table, max_pred, max_gt, thresholds, more=()):
    """What ``match_instances`` and ``match_instances_boundary`` check alike once their label maps are int32 [N, H, W] of one shape
    (each words and orders those errors its own way): the table, P, G, the cell bound, the thresholds, and that every tensor is on
    ``pred_labels``' HIP device -- ``more``: (name, map or ``None``) pairs of further maps.  Returns a namespace: the two maps and the table detached and contiguous, ``dims`` =
    (N, H, W, P, G), the table's pointer and ``rows``, and ``match_thresholds``' ``fr``, ``nums``, ``den`` with ``T``."""
    N, H, W = pred_labels.shape
    rows = 0
    if pred_table is not None:
        if not isinstance(pred_table, torch.Tensor) or pred_table.dtype != torch.int64:
            raise ValueError("pred_table must be an int64 tensor")
        if pred_table.dim() == 2:
            pred_table = pred_table.unsqueeze(0)
        if pred_table.dim() != 3 or pred_table.shape[0] != N or pred_table.shape[1] < 1 or pred_table.shape[2] != _lib.INST_FIELDS:
            raise ValueError(f"need pred_table [N = {N}, rows >= 1, {_lib.INST_FIELDS}], got {tuple(pred_table.shape)}")
        rows = int(pred_table.shape[1])
    P = _id_bound((rows or 64) if max_pred is None else max_pred, "max_pred")
    G = _id_bound(64 if max_gt is None else max_gt, "max_gt")
    if N * (P + 1) * (G + 1) > _lib.IM_MAX_CELLS:
        raise ValueError(f"max_pred = {P} and max_gt = {G} for {N} images exceed {_lib.IM_MAX_CELLS} table cells")
    fr, nums, den = match_thresholds(thresholds)
    _lib.require_device(pred_labels, "pred_labels")
    dev = pred_labels.device
    for name, t in (("gt_labels", gt_labels), ("pred_table", pred_table), *more):
        if t is not None:
            _lib.require_device(t, name)
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, pred_labels on {dev}")
    if pred_table is not None:
        pred_table = pred_table.detach().contiguous()
    return SimpleNamespace(pred_labels=pred_labels.detach().contiguous(), gt_labels=gt_labels.detach().contiguous(), pred_table=pred_table,
                           table_ptr=None if pred_table is None else _ptr(pred_table), rows=rows, dims=(N, H, W, P, G), fr=fr, nums=nums,
                           den=den, T=len(nums))


def _match_buffers(entry, m, row_fields, gt_fields):
    """The workspace of ``entry`` (``camo_inst_match`` or ``camo_boundary_match``) for ``_match_inputs``' ``m`` and the call's six
    output tensors, "pred_rows" [N, P, *row_fields] and "gt_area" [N, G, *gt_fields]: (the device, ws, the dict).  A step
    of its own because ``match_instances_boundary`` makes its boundary maps, which may raise, between the checks and this."""
    N, H, W, P, G = m.dims
    dev = m.pred_labels.device
    ws, _ = workspace(entry + "_workspace_bytes", N, H, W, P, G, m.T, device=dev,
                      refuse=lambda: ValueError(f"{entry} does not support N = {N}, H = {H}, W = {W}, P = {P}, G = {G}, T = {m.T}"))
    shapes = {"inter": (N, P + 1, G + 1), "pred_rows": (N, P, *row_fields), "gt_area": (N, G, *gt_fields), "match": (N, m.T, P),
              "gt_match": (N, m.T, G), "counts": (N, _lib.IM_COUNTS)}
    return dev, ws, {k: torch.empty(*shape, dtype=torch.int32, device=dev) for k, shape in shapes.items()}


@torch.no_grad()
def match_instances(pred_labels, gt_labels, pred_table=None, max_pred=None, max_gt=None, thresholds=COCO):
    """``camo_inst_match``: ``pred_labels`` and ``gt_labels`` int32 [N, H, W] (or [H, W]), 0 on background, as ``mask_instances``
    writes them; ``pred_table`` its int64 [N, rows, 8] table (the score order; ``None``: the order is by id).  Returns {"inter":
    int32 [N, P + 1, G + 1] (pixels of every pair), "pred_rows": int32 [N, P, 4] = (area, rank, ground-truth id of highest IoU, the
    intersection with it), "gt_area": int32 [N, G], "match": int32 [N, T, P] (the ground-truth id every predicted id is matched to
    at threshold k, or 0), "gt_match": int32 [N, T, G], "counts": int32 [N, 4] = (pixels with a predicted label above P, pixels with
    a ground-truth label above G, predicted ids in use, ground-truth ids in use), "thresholds": the T Fractions}, the tensors on
    the device, no host synchronisation.  P = ``max_pred`` (default: the table's rows, 64 without a table), G = ``max_gt`` (64)."""
    if not isinstance(pred_labels, torch.Tensor) or not isinstance(gt_labels, torch.Tensor):
        raise ValueError("pred_labels and gt_labels must be tensors")
    if pred_labels.dim() == 2:
        pred_labels = pred_labels.unsqueeze(0)
    if gt_labels.dim() == 2:
        gt_labels = gt_labels.unsqueeze(0)
    if pred_labels.dim() != 3 or pred_labels.numel() == 0:
        raise ValueError(f"need pred_labels [N, H, W] or [H, W] with at least one pixel, got {tuple(pred_labels.shape)}")
    if tuple(gt_labels.shape) != tuple(pred_labels.shape):
        raise ValueError(f"need gt_labels of pred_labels' shape {tuple(pred_labels.shape)}, got {tuple(gt_labels.shape)}")
    for t, name in ((pred_labels, "pred_labels"), (gt_labels, "gt_labels")):
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, got {t.dtype}")
    m = _match_inputs(pred_labels, gt_labels, pred_table, max_pred, max_gt, thresholds)
    dev, ws, out = _match_buffers("camo_inst_match", m, (4,), ())
    call("camo_inst_match", dev, _ptr(m.pred_labels), _ptr(m.gt_labels), *m.dims, m.table_ptr, m.rows, (C.c_int32 * m.T)(*m.nums), m.den, m.T,
         _ptr(out["inter"]), _ptr(out["pred_rows"]), _ptr(out["gt_area"]), _ptr(out["match"]), _ptr(out["gt_match"]),
         _ptr(out["counts"]), _ptr(ws), ws.numel(), _stream_ptr(dev))
    return {**out, "thresholds": m.fr}


def _ratio(a, b):
    return a / b if b else 0.0


def instance_match_records(out):
    """The per-image ratios of include/camo_inst_match.h from ``match_instances``' dict (device tensors cost the one host copy), in
    float64 from the exact integers.  Per image a dict {"thresholds": the T Fractions, "per_threshold": [{"tp", "fp", "fn",
    "precision", "recall", "f1"}] (a ratio with a zero denominator is 0.0), "predictions": [{"id", "area", "rank", "best_gt",
    "best_iou", "matches": the matched ground-truth id per threshold (0: none)} for every predicted id in use, in id order],
    "n_pred", "n_gt": the ids in use, "pq", "sq", "rq": panoptic quality from the first threshold equal to 1/2, over its matched pairs
    with 2 i > u -- sq the mean IoU of those pairs, rq = tp / (tp + fp / 2 + fn / 2), pq = sq rq; ``None`` when no threshold is 1/2
    or the image holds no instance on either side --, "truncated_pred", "truncated_gt": pixels carried a label past the tables}."""
    fr = tuple(out["thresholds"])
    names = ("inter", "pred_rows", "gt_area", "match", "gt_match", "counts")
    tensors = [out[k] for k in names]
    flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()      # (the one copy)
    arrays, at = {}, 0
    for k, t in zip(names, tensors):
        arrays[k] = flat[at:at + t.numel()].reshape(tuple(t.shape))
        at += t.numel()
    inter, rows, gt_area, match, counts = arrays["inter"], arrays["pred_rows"], arrays["gt_area"], arrays["match"], arrays["counts"]
    N, T, P = match.shape
    half = next((k for k, f in enumerate(fr) if f == Fraction(1, 2)), None)
    records = []
    for n in range(N):
        n_pred, n_gt = int(counts[n, 2]), int(counts[n, 3])
        per = []
        for k in range(T):
            tp = int((match[n, k] > 0).sum())
            fp, fn = n_pred - tp, n_gt - tp
            pr, rc = _ratio(tp, tp + fp), _ratio(tp, tp + fn)
            per.append({"tp": tp, "fp": fp, "fn": fn, "precision": pr, "recall": rc, "f1": _ratio(2 * pr * rc, pr + rc)})
        preds = []
        for p in range(1, P + 1):
            area, rank, best, bi = (int(v) for v in rows[n, p - 1])
            if area == 0:
                continue
            iou = bi / (area + int(gt_area[n, best - 1]) - bi) if best else 0.0
            preds.append({"id": p, "area": area, "rank": rank, "best_gt": best, "best_iou": iou, "matches": [int(match[n, k, p - 1]) for k in range(T)]})
        pq = sq = rq = None
        if half is not None and n_pred + n_gt:
            ious = []
            for p in range(1, P + 1):
                g = int(match[n, half, p - 1])
                if g:
                    i = int(inter[n, p, g])
                    u = int(rows[n, p - 1, 0]) + int(gt_area[n, g - 1]) - i
                    if 2 * i > u:
                        ious.append(i / u)
            tp = len(ious)
            sq = _ratio(sum(ious), tp)
            rq = tp / (tp + (n_pred - tp) / 2 + (n_gt - tp) / 2)
            pq = sq * rq
        records.append({"thresholds": fr, "per_threshold": per, "predictions": preds, "n_pred": n_pred, "n_gt": n_gt, "pq": pq, "sq": sq,
                        "rq": rq, "truncated_pred": bool(counts[n, 0] > 0), "truncated_gt": bool(counts[n, 1] > 0)})
    return records


def match_options(match, instances=True, have_masks=True, coco=False):
    """The pipeline's ``match`` keyword -- ``None`` (off), ``True`` or a dict with any of "thresholds" (COCO), "gt_labels" (int32
    ground-truth ids; default: the connected components of the ground-truth mask), "gt_rles" (the ground-truth ids as COCO RLEs per
    image, ``rle.decode_rles``' argument; not together with "gt_labels"), "gt_segmentations" (per image a list of COCO
    ``segmentation`` fields, polygons or RLEs, or (segmentation, id) pairs: ``polygons.decode_segmentations``' argument; not together
    with either) and "max_gt" (64) -- as a dict with all five, or ``None``; the ``ValueError`` of a bad one by name, before anything
    touches the device.  ``coco=True`` (``detect_camouflage_directory``) also takes "gt_coco", a COCO annotations file, in the place of
    the other three."""
    if match is None or match is False:
        return None
    if match is True:
        match = {}
    known = {"thresholds", "gt_labels", "gt_rles", "max_gt", "gt_segmentations"} | ({"gt_coco"} if coco else set())
    if not isinstance(match, dict) or set(match) - known:
        raise ValueError('match must be None, True or a dict with any of "thresholds", "gt_labels", "gt_rles", "max_gt", "gt_segmentations"'
                         + (', "gt_coco"' if coco else "") + f", got {match!r}")
    if not instances:
        raise ValueError("match needs instances=True: the predicted instances are what it matches")
    opts = {"thresholds": match.get("thresholds", COCO), "gt_labels": match.get("gt_labels"), "gt_rles": match.get("gt_rles"),
            "max_gt": match.get("max_gt", 64), "gt_segmentations": match.get("gt_segmentations")}
    if coco:
        opts["gt_coco"] = match.get("gt_coco")
    if opts["gt_labels"] is not None and opts["gt_rles"] is not None:
        raise ValueError('match takes "gt_labels" or "gt_rles", not both')
    if opts["gt_segmentations"] is not None and (opts["gt_labels"] is not None or opts["gt_rles"] is not None):
        raise ValueError('match takes one of "gt_labels", "gt_rles" and "gt_segmentations", not two')
    if opts.get("gt_coco") is not None and any(opts[k] is not None for k in ("gt_labels", "gt_rles", "gt_segmentations")):
        raise ValueError('match takes "gt_coco" or one of "gt_labels", "gt_rles" and "gt_segmentations", not both')
    if opts["gt_rles"] is not None and (not isinstance(opts["gt_rles"], (list, tuple)) or not opts["gt_rles"]):
        raise ValueError('match["gt_rles"] must be a non-empty list with one list of RLEs per image')
    if opts["gt_segmentations"] is not None and (not isinstance(opts["gt_segmentations"], (list, tuple)) or not opts["gt_segmentations"]):
        raise ValueError('match["gt_segmentations"] must be a non-empty list with one list of COCO segmentations per image')
    if opts.get("gt_coco") is not None and not isinstance(opts["gt_coco"], (str, os.PathLike, dict)):
        raise ValueError('match["gt_coco"] must be the path of a COCO annotations file or its dict')
    if all(opts.get(k) is None for k in ("gt_labels", "gt_rles", "gt_segmentations", "gt_coco")) and not have_masks:
        raise ValueError('match needs ground truth: gt_masks, match["gt_labels"] or match["gt_rles"]')
    match_thresholds(opts["thresholds"])
    _id_bound(opts["max_gt"], 'match["max_gt"]')
    return opts


def ground_truth_labels(gt_masks, connectivity=8, max_gt=64):
    """The instances of ground-truth masks [N, H, W] (bool, or uint8 positive above 127): ``mask_instances``' labels of the mask's
    connected components with ``connectivity``, ``min_area=0`` and no hole filling."""
    positive = gt_masks if gt_masks.dtype == torch.bool else gt_masks > 127
    return mask_instances(positive.to(torch.float32), 0.5, connectivity, 0, False, max_gt)["labels"]


@torch.no_grad()
def match_detected(pred_labels, pred_table, gt_labels, opts):
    """``match_instances`` and ``instance_match_records`` together, for the pipeline: (records, ``match_instances``' dict).  The
    tables hold ``pred_table``'s rows and ``opts["max_gt"]`` ground-truth ids; when an image carries a label past either, the call
    is made once more with the tables sized to the largest labels (at most CAMO_IM_MAX_IDS), as ``detect_instances`` does."""
    return _match_detected(partial(match_instances, thresholds=opts["thresholds"]), instance_match_records, pred_labels, pred_table, gt_labels,
                           opts["max_gt"])


def _match_detected(match, records, pred_labels, pred_table, gt_labels, max_gt, keep=()):
    """``match(pred_labels, gt_labels, pred_table, P, G)`` and ``records`` of its dict, with the second call of ``match_detected``;
    that call is given the first one's ``keep`` entries as keywords."""
    gt_labels = torch.as_tensor(gt_labels)
    if gt_labels.dim() == 2:
        gt_labels = gt_labels.unsqueeze(0)
    gt_labels = gt_labels.to(device=pred_labels.device, dtype=torch.int32)
    P, G = min(int(pred_table.shape[1]), _lib.IM_MAX_IDS), int(max_gt)
    tables = match(pred_labels, gt_labels, pred_table, P, G)
    rec = records(tables)
    if any(r["truncated_pred"] or r["truncated_gt"] for r in rec):
        P2 = min(max(P, int(pred_labels.max())), _lib.IM_MAX_IDS)
        G2 = min(max(G, int(gt_labels.max())), _lib.IM_MAX_IDS)
        if (P2, G2) != (P, G):
            tables = match(pred_labels, gt_labels, pred_table, P2, G2, **{k: tables[k] for k in keep})
            rec = records(tables)
    return rec, tables


def average_precision(scored, n_gt):
    """COCO's 101-point interpolated average precision of ``scored`` = [(score, is true positive)] against ``n_gt`` ground-truth
    instances: sorted by score descending (stable), the precision envelope taken from the right, and the recall r = j / 100 sampled
    at the first index whose recall is at least r (0 where none is).  ``None`` when ``n_gt`` is 0."""
    if n_gt == 0:
        return None
    ranked = sorted(scored, key=lambda s: -s[0])      # (sorted is stable: equal scores keep their insertion order)
    tps, prec, tp = [], [], 0
    for j, (_, hit) in enumerate(ranked):
        tp += 1 if hit else 0
        tps.append(tp)
        prec.append(tp / (j + 1))
    for j in range(len(prec) - 2, -1, -1):
        prec[j] = max(prec[j], prec[j + 1])
    total, at = 0.0, 0
    for j in range(101):
        while at < len(tps) and tps[at] * 100 < j * n_gt:      # recall >= j / 100, in integers
            at += 1
        total += prec[at] if at < len(tps) else 0.0
    return total / 101


class InstanceAP:
    """Dataset average precision from ``instance_match_records``' records.  ``add(records, scores)`` takes the records of some images
    and, per image, the scores of its predicted ids (``scores[i][p - 1]`` is id p's: ``[r["score"] for r in instances]`` of
    ``instance_records``); ``result()`` gives {"AP": the mean over the thresholds of ``average_precision``, "AP50", "AP75" (where
    1/2 and 3/4 are among the thresholds), "AR": the mean recall, "per_threshold": the AP of every threshold, "n_gt", "n_pred"}.
    "AP" and the others are ``None`` when no ground-truth instance was added."""

    def __init__(self):
        self.thresholds = None
        self.scored = []          # per threshold [(score, is true positive)]
        self.n_gt = 0
        self.n_pred = 0

    def add(self, records, scores):
        if len(records) != len(scores):
            raise ValueError(f"{len(records)} records and {len(scores)} score lists")
        for rec, sc in zip(records, scores):
            if self.thresholds is None:
                self.thresholds = tuple(rec["thresholds"])
                self.scored = [[] for _ in self.thresholds]
            elif tuple(rec["thresholds"]) != self.thresholds:
                raise ValueError("records of different thresholds")
            for pred in rec["predictions"]:
                if pred["id"] > len(sc):
                    raise ValueError(f"no score for predicted id {pred['id']}: {len(sc)} scores")
                for k, g in enumerate(pred["matches"]):
                    self.scored[k].append((float(sc[pred["id"] - 1]), g > 0))
            self.n_gt += rec["n_gt"]
            self.n_pred += rec["n_pred"]
        return self

    def result(self):
        out = {"AP": None, "AR": None, "per_threshold": None, "n_gt": self.n_gt, "n_pred": self.n_pred}
        if self.n_gt == 0 or self.thresholds is None:
            return out
        aps = [average_precision(s, self.n_gt) for s in self.scored]
        out.update({"AP": sum(aps) / len(aps), "per_threshold": aps,
                    "AR": sum(sum(1 for _, hit in s if hit) / self.n_gt for s in self.scored) / len(aps)})
        for name, f in (("AP50", Fraction(1, 2)), ("AP75", Fraction(3, 4))):
            if f in self.thresholds:
                out[name] = aps[self.thresholds.index(f)]
        return out
