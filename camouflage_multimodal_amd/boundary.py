"""Boundary IoU and Boundary AP on MI355X (include/camo_boundary.h): does a predicted object's CONTOUR lie where the
ground truth's does?

Mask IoU grows with object area, so it barely sees the contour of a large object; Boundary IoU (Cheng et al., CVPR 2021) is the IoU
of the two boundary regions -- an instance minus its erosion by ``d`` iterations of a 3 x 3 square, d = round(0.02 x image diagonal)
-- and Boundary AP runs COCO's greedy matching on min(mask IoU, boundary IoU).  ``boundary_labels`` runs ``camo_boundary_labels`` on a
label map, ``match_instances_boundary`` runs ``camo_boundary_match`` and returns device tensors, ``boundary_match_records`` takes the
ratios from the integers on the host with the keys of ``instance_match_records`` -- so ``InstanceAP`` fed with them gives Boundary AP
-- and ``boundary_iou`` is the semantic-segmentation form on binary masks.
PARITY UNPINNED: the header's text is the definition (restated in numpy in tests/boundary_ref.py).  There is no CPU path: tensors
that are not on a HIP device raise.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from fractions import Fraction
from functools import partial

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, label_map, workspace
from .instance_match import COCO, _match_buffers, _match_detected, _match_inputs, _ratio, instance_match_records, match_instances

RATIO = Fraction(1, 50)


def _ratio_fraction(ratio):
    if isinstance(ratio, bool) or not isinstance(ratio, (numbers.Rational, float)):
        raise ValueError(f"ratio must be a Fraction, an integer or a float in (0, 1], got {ratio!r}")
    if isinstance(ratio, float):
        if not math.isfinite(ratio):
            raise ValueError(f"ratio must be a Fraction, an integer or a float in (0, 1], got {ratio!r}")
        ratio = Fraction(ratio).limit_denominator(1 << 20)
    ratio = Fraction(ratio)
    if not 0 < ratio <= 1:
        raise ValueError(f"ratio must be in (0, 1], got {ratio!r}")
    return ratio


def _side(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return int(v)


def boundary_distance(H, W, ratio=RATIO):
    """The erosion distance of an H x W image: ``ratio`` times its diagonal, rounded half up, at least 1 -- in exact integers:
    max(1, (isqrt(4 num^2 (H^2 + W^2)) + den) // (2 den)) for ratio = num / den.  256 x 256 -> 7, 480 x 640 -> 16."""
    H, W, r = _side(H, "H"), _side(W, "W"), _ratio_fraction(ratio)
    num, den = r.numerator, r.denominator
    return max(1, (math.isqrt(4 * num * num * (H * H + W * W)) + den) // (2 * den))


def _distance(distance, ratio, H, W):
    if distance is None:
        distance = boundary_distance(H, W, ratio)
    if isinstance(distance, bool) or not isinstance(distance, numbers.Integral) or not 1 <= distance <= _lib.BD_MAX_DISTANCE:
        raise ValueError(f"distance must be an integer in [1, {_lib.BD_MAX_DISTANCE}], got {distance!r}")
    return int(distance)


@torch.no_grad()
def boundary_labels(labels, distance=None, ratio=RATIO):
    """``camo_boundary_labels``: ``labels`` int32 [N, H, W] (or [H, W]), 0 on background -> int32 [N, H, W], every instance's id on
    its boundary region and 0 elsewhere.  ``distance``: the erosion distance d (default ``boundary_distance(H, W, ratio)``).  Two
    launches, no host synchronisation."""
    labels = label_map(labels, "labels")
    N, H, W = labels.shape
    d = _distance(distance, ratio, H, W)
    _lib.require_device(labels, "labels")
    labels = labels.detach().contiguous()
    dev = labels.device
    ws, nbytes = workspace("camo_boundary_labels_workspace_bytes", N, H, W, d, device=dev,
                           refuse=lambda: ValueError(f"camo_boundary_labels does not support N = {N}, H = {H}, W = {W}, d = {d}"))
    out = torch.empty_like(labels)
    call("camo_boundary_labels", dev, _ptr(labels), N, H, W, d, _ptr(out), _ptr(ws), nbytes, _stream_ptr(dev))
    return out


@torch.no_grad()
def match_instances_boundary(pred_labels, gt_labels, pred_table=None, max_pred=None, max_gt=None, thresholds=COCO, distance=None, ratio=RATIO,
                             pred_boundary=None, gt_boundary=None):
    """``camo_boundary_match``: ``match_instances`` under min(mask IoU, boundary IoU).  ``pred_boundary`` / ``gt_boundary``: the
    boundary maps when the caller has them (ground truth is eroded once per dataset); otherwise ``boundary_labels`` with ``distance``
    (default ``boundary_distance(H, W, ratio)``).  Returns ``match_instances``' dict with "inter_bd" int32 [N, P + 1, G + 1] beside
    "inter", "pred_rows" int32 [N, P, 6] = (area, rank, ground-truth id of highest combined IoU, the mask intersection with it,
    boundary area, the boundary intersection with it), "gt_area" int32 [N, G, 2] = (area, boundary area), "pred_boundary",
    "gt_boundary" (the maps) and "distance" (``None`` when both maps were given without one).  No host synchronisation."""
    pred_labels, gt_labels = label_map(pred_labels, "pred_labels"), label_map(gt_labels, "gt_labels")
    if tuple(gt_labels.shape) != tuple(pred_labels.shape):
        raise ValueError(f"need gt_labels of pred_labels' shape {tuple(pred_labels.shape)}, got {tuple(gt_labels.shape)}")
    N, H, W = pred_labels.shape
    given = {"pred_boundary": pred_boundary, "gt_boundary": gt_boundary}
    for name, t in given.items():
        if t is not None:
            given[name] = t = label_map(t, name)
            if tuple(t.shape) != (N, H, W):
                raise ValueError(f"need {name} of pred_labels' shape {(N, H, W)}, got {tuple(t.shape)}")
    d = None
    if distance is not None or None in given.values():
        d = _distance(distance, ratio, H, W)
    m = _match_inputs(pred_labels, gt_labels, pred_table, max_pred, max_gt, thresholds, given.items())
    pred_bd = boundary_labels(m.pred_labels, d) if given["pred_boundary"] is None else given["pred_boundary"].detach().contiguous()
    gt_bd = boundary_labels(m.gt_labels, d) if given["gt_boundary"] is None else given["gt_boundary"].detach().contiguous()
    dev, ws, out = _match_buffers("camo_boundary_match", m, (_lib.BD_ROW_FIELDS,), (_lib.BD_GT_FIELDS,))
    inter_bd = torch.empty_like(out["inter"])
    call("camo_boundary_match", dev, _ptr(m.pred_labels), _ptr(m.gt_labels), _ptr(pred_bd), _ptr(gt_bd), *m.dims, m.table_ptr, m.rows,
         (C.c_int32 * m.T)(*m.nums), m.den, m.T, _ptr(out["inter"]), _ptr(inter_bd), _ptr(out["pred_rows"]), _ptr(out["gt_area"]),
         _ptr(out["match"]), _ptr(out["gt_match"]), _ptr(out["counts"]), _ptr(ws), ws.numel(), _stream_ptr(dev))
    return {"inter": out["inter"], "inter_bd": inter_bd, **out, "thresholds": m.fr, "pred_boundary": pred_bd, "gt_boundary": gt_bd,
            "distance": d}


def boundary_match_records(out):
    """``instance_match_records`` of ``match_instances_boundary``'s dict: the same keys per image, taken under the combined IoU -- so
    ``InstanceAP().add(records, scores).result()`` IS Boundary AP --, "best_iou" the combined IoU with "best_gt"; and more: per
    prediction "boundary_area", "best_boundary_iou" and "best_mask_iou", per image "distance".  Panoptic quality is not taken under the
    combined IoU: "pq", "sq" and "rq" are ``None``."""
    rows, gt_area = out["pred_rows"], out["gt_area"]
    # the base records from the first four fields: the matches and counts in them are already the combined ones
    records = instance_match_records(dict(out, pred_rows=rows[..., :4], gt_area=gt_area[..., 0]))
    rows, gt_area = rows.cpu().numpy(), gt_area.cpu().numpy()
    for n, rec in enumerate(records):
        rec["pq"] = rec["sq"] = rec["rq"] = None
        rec["distance"] = out.get("distance")
        for pred in rec["predictions"]:
            area, _, best, i, b_area, ib = (int(v) for v in rows[n, pred["id"] - 1])
            mask_iou = boundary_iou_ = 0.0
            if best:
                mask_iou = _ratio(i, area + int(gt_area[n, best - 1, 0]) - i)
                boundary_iou_ = _ratio(ib, b_area + int(gt_area[n, best - 1, 1]) - ib)
            pred.update({"boundary_area": b_area, "best_boundary_iou": boundary_iou_, "best_mask_iou": mask_iou,
                         "best_iou": min(mask_iou, boundary_iou_)})
    return records


@torch.no_grad()
def boundary_iou(pred_masks, gt_masks, distance=None, ratio=RATIO):
    """Boundary IoU of binary masks, the semantic-segmentation form: ``pred_masks`` and ``gt_masks`` bool [N, H, W] (or [H, W]) as
    label 1, through ``boundary_labels`` and ``match_instances`` with one id on either side.  Per image {"boundary_iou", "mask_iou"
    (0.0 when the union is empty), "distance"}; the one host copy is the two 2 x 2 tables'."""
    for t, name in ((pred_masks, "pred_masks"), (gt_masks, "gt_masks")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bool:
            raise ValueError(f"{name} must be a bool tensor")
    if pred_masks.dim() == 2:
        pred_masks = pred_masks.unsqueeze(0)
    if gt_masks.dim() == 2:
        gt_masks = gt_masks.unsqueeze(0)
    if pred_masks.dim() != 3 or pred_masks.numel() == 0:
        raise ValueError(f"need pred_masks [N, H, W] or [H, W] with at least one pixel, got {tuple(pred_masks.shape)}")
    if tuple(gt_masks.shape) != tuple(pred_masks.shape):
        raise ValueError(f"need gt_masks of pred_masks' shape {tuple(pred_masks.shape)}, got {tuple(gt_masks.shape)}")
    N, H, W = pred_masks.shape
    d = _distance(distance, ratio, H, W)
    _lib.require_device(pred_masks, "pred_masks")
    _lib.require_device(gt_masks, "gt_masks")
    pl, gl = pred_masks.to(torch.int32), gt_masks.to(torch.int32)
    half = (Fraction(1, 2),)
    mask = match_instances(pl, gl, None, 1, 1, half)["inter"]
    bd = match_instances(boundary_labels(pl, d), boundary_labels(gl, d), None, 1, 1, half)["inter"]
    tables = torch.stack([mask, bd]).cpu().numpy()
    out = []
    for n in range(N):
        ious = []
        for t in tables[:, n]:
            i = int(t[1, 1])
            ious.append(_ratio(i, int(t[1].sum()) + int(t[:, 1].sum()) - i))
        out.append({"boundary_iou": ious[1], "mask_iou": ious[0], "distance": d})
    return out


def boundary_options(boundary, match):
    """The pipeline's ``boundary`` keyword -- ``None`` (off), ``True`` or a dict with any of "ratio" (1/50) and "distance" (an integer
    in the place of ratio x diagonal) -- as a dict with both, or ``None``; the ``ValueError`` of a bad one by name, before anything
    touches the device.  ``match``: ``match_options``' result -- the matching is what it extends."""
    if boundary is None or boundary is False:
        return None
    if boundary is True:
        boundary = {}
    if not isinstance(boundary, dict) or set(boundary) - {"ratio", "distance"}:
        raise ValueError(f'boundary must be None, True or a dict with any of "ratio", "distance", got {boundary!r}')
    if match is None:
        raise ValueError("boundary needs match: the matching under the combined IoU is what it adds")
    opts = {"ratio": _ratio_fraction(boundary.get("ratio", RATIO)), "distance": boundary.get("distance")}
    if opts["distance"] is not None:
        _distance(opts["distance"], opts["ratio"], 1, 1)
    return opts


@torch.no_grad()
def match_detected_boundary(pred_labels, pred_table, gt_labels, opts, boundary):
    """``match_instances_boundary`` and ``boundary_match_records`` together, for the pipeline: (records, the dict).  ``opts``:
    ``match_options``' dict, ``boundary``: ``boundary_options``'.  The tables are sized as ``match_detected`` sizes them, with the
    same second call when an image carries a label past either; the boundary maps are made once."""
    match = partial(match_instances_boundary, thresholds=opts["thresholds"], distance=boundary["distance"], ratio=boundary["ratio"])
    return _match_detected(match, boundary_match_records, pred_labels, pred_table, gt_labels, opts["max_gt"], ("pred_boundary", "gt_boundary"))
