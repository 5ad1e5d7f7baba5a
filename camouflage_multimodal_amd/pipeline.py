"""The detection pipeline on MI355X: images in, masks, instances, matches and benchmark measures out.

``detect_camouflage_batch`` (and the reference's name for one image, ``detect_camouflage``) runs the detector on a batch of one
size; ``detect_camouflage_ragged`` takes uint8 images of mixed sizes through it and back to their own sizes, and
``detect_camouflage_directory`` takes a folder of files through that.  Everything here is host-side plumbing on top of the kernel
bindings -- region_graph.py, rg_detect.py, seg_measures.py, instances.py, instance_match.py, boundary.py, rle.py, polygons.py, contours.py,
resize.py, refine.py -- and what the entry points share is stated once: ``_by_size`` (images of equal size share a library call) and
``_match_ground_truth`` (where the ground-truth ids of ``match`` come from).  This module imports all of those and is imported by
rg_finetune.py only.  There is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib, boundary as _boundary, contours as _contours, instance_match as _match, instances as _instances, polygons as _polygons, refine as _refine, rle as _rle, seg_measures, \
    split as _split
from .region_graph import _as_tensor, _image_batch, create_region_graphs_from_segments, slic_label_bound, slic_segments
from .resize import _device, _mask_list, _packed, _ragged, resize_batch, resize_to_sizes
from .rg_detect import paint_regions, segmentation_counts, segmentation_metrics

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp")
GT_SOURCES = (("gt_rles", "lists"), ("gt_segmentations", "lists"), ("gt_labels", "maps"))      # of ``match``: at most one is given


def _by_size(shapes, call, results=None):
    """What the per-image steps of mixed sizes share: ``shapes`` (per image its (H, W), or a tensor whose shape is that) are grouped by
    size, in order of first appearance with the indices ascending inside a group, ``call(idx, (H, W))`` is made once per group and
    what it returns for the group's j-th image goes to place idx[j].  ``call`` returns one indexable result (``results=None``: one
    list comes back) or a tuple of ``results`` of them (a tuple of as many lists)."""
    shapes = [tuple(s.shape) if hasattr(s, "shape") else tuple(s) for s in shapes]
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    out = [[None] * len(shapes) for _ in range(1 if results is None else results)]
    for size, idx in groups.items():
        got = call(idx, size)
        for filled, part in zip(out, (got,) if results is None else got):
            for j, i in enumerate(idx):
                filled[i] = part[j]
    return out[0] if results is None else tuple(out)


def _stack(items, idx):
    return torch.stack([items[i] for i in idx])


def _check_pairs(maps, truths, what, truth):
    for i, (p, g) in enumerate(zip(maps, truths)):
        if tuple(p.shape) != tuple(g.shape):
            raise ValueError(f"image {i}: the {what} is {tuple(p.shape)}, its {truth} {tuple(g.shape)}")


def _score(preds, gts, threshold, cod, curves=False):
    """``segmentation_metrics`` (and ``seg_measures.cod_metrics``) of every fp32 [H_i, W_i] map against its uint8 mask of the same
    size; maps of equal size share a call.  Returns (metrics list, cod list or None) in the maps' order."""
    _check_pairs(preds, gts, "map", "mask")

    def score(idx, size):
        p, g = _stack(preds, idx), _stack(gts, idx)
        metrics = segmentation_metrics(segmentation_counts(p, g, threshold), *size)
        return (metrics, seg_measures.cod_metrics(p, g, curves)) if cod else (metrics,)

    out = _by_size(preds, score, 2 if cod else 1)
    return out[0], out[1] if cod else None


def _native_matches(labels, tables, gt_labels, opts):
    """``instance_match.match_detected`` of every int32 [H_i, W_i] label map against its ground-truth ids; maps of equal size share
    a call.  Returns (records, tables), two lists in the maps' order (a table dict holds the image's own rows)."""
    _check_pairs(labels, gt_labels, "label map", "ground truth")

    def matched(idx, _):
        r, t = _match.match_detected(_stack(labels, idx), _stack(tables, idx),
                                     torch.stack([torch.as_tensor(gt_labels[i]).to(labels[i].device, torch.int32) for i in idx]), opts)
        return r, _per_image(t, len(idx))

    return _by_size(labels, matched, 2)


def _per_image(tables, n):
    return [{k: (v[j] if isinstance(v, torch.Tensor) else v) for k, v in tables.items()} for j in range(n)]


def _native_boundary_matches(labels, tables, gt_labels, opts, boundary):
    """``_native_matches`` under the combined IoU (``boundary.match_detected_boundary``): a size group's distance comes from its own
    H and W."""
    _check_pairs(labels, gt_labels, "label map", "ground truth")

    def matched(idx, _):
        r, t = _boundary.match_detected_boundary(_stack(labels, idx), _stack(tables, idx),
                                                 torch.stack([torch.as_tensor(gt_labels[i]).to(labels[i].device, torch.int32) for i in idx]), opts, boundary)
        return r, _per_image(t, len(idx))

    return _by_size(labels, matched, 2)


def _positive(gt):
    return gt if gt.dtype == torch.bool else gt > 127


def _native_boundary_ious(masks, truths, boundary):
    """``boundary.boundary_iou`` of every bool [H_i, W_i] mask against its ground-truth mask; masks of equal size share a call."""
    _check_pairs(masks, truths, "mask", "ground-truth mask")
    return _by_size(masks, lambda idx, _: _boundary.boundary_iou(_stack(masks, idx), _positive(_stack(truths, idx)), boundary["distance"], boundary["ratio"]))


def _split_found(found, prob, split):
    """``split.split_detected`` of detected instances (``detect_instances``' "instances" and "labels") with the probability they came
    from; ``split``: ``split_options``' dict.  An image with more ids than a label map may hold for the splitter raises."""
    most = max(r["count"] for r in found["instances"])
    if most > _lib.IM_MAX_IDS:
        raise ValueError(f"split takes at most {_lib.IM_MAX_IDS} instances per image, an image holds {most}: raise min_area")
    return _split.split_detected(found["labels"], prob, split)


def _check_sources(match, n, noun):
    for key, what in GT_SOURCES:
        if match[key] is not None and len(match[key]) != n:
            raise ValueError(f'match["{key}"] holds {len(match[key])} {what} for {n} {noun}')


def _match_ground_truth(match, n, noun, sizes, masks, connectivity, device):
    """The ground-truth ids that ``match`` (``instance_match.match_options``' dict) asks for, for ``n`` images (``noun`` in the
    messages) of ``sizes``: n int32 label maps [H_i, W_i], from "gt_rles" (``rle.decode_rles``), else "gt_segmentations"
    (``polygons.decode_segmentations``), else "gt_labels" as they are, else the connected components of ``masks`` (n masks [H_i, W_i];
    ``instance_match.ground_truth_labels`` with ``connectivity``).  Images of equal size share a call, and a decoder's messages keep
    the caller's image numbers."""
    _check_sources(match, n, noun)
    for key, decode in (("gt_rles", _rle.decode_rles), ("gt_segmentations", _polygons.decode_segmentations)):
        if match[key] is not None:
            return _by_size(sizes, lambda idx, size: decode([match[key][i] for i in idx], *size, device, image_numbers=idx))
    if match["gt_labels"] is not None:
        return match["gt_labels"]
    return _by_size(sizes, lambda idx, _: _match.ground_truth_labels(_stack(masks, idx), connectivity, match["max_gt"]))


@torch.no_grad()
def detect_camouflage_batch(rg_model, images, gt_masks=None, n_segments=500, threshold=0.5, device="cuda", cod_metrics=False,
                            instances=False, min_area=0, fill_holes=False, connectivity=8, refine=None, *, match=None, rle=False, boundary=None,
                            split=False, polygons=False):
    """``detect_camouflage`` of the reference (models/region_graph/test.py) for a batch: ``images`` [N, H, W, 3] float in [0, 1] ->
    {"prob_maps": fp32 [N, 3, H, W] (mask, instance, edge probability of every pixel's superpixel), "mask": bool [N, H, W]
    (mask probability > ``threshold``), "node_probs": [n, 3], "graphs": RegionGraphBatch, "segments": int32 [N, H, W],
    "region_map": int32 [N, label_bound]}, all on the device, plus "metrics" (``segmentation_metrics`` of the mask probability
    against ``gt_masks`` [N, H, W] uint8 / bool) when ``gt_masks`` is given.  Host synchronisations: the graph sizes read-back and,
    with ``gt_masks``, one [N, 5] copy.  ``cod_metrics=True`` (needs ``gt_masks``) adds "cod_metrics": per image the dict of
    ``seg_measures.cod_metrics`` -- S-alpha, E-phi, the F-beta numbers, MAE on the 8-bit map and ``wf`` -- of the mask probability,
    at the price of one more host copy, of the two small tables.  ``instances=True`` adds the objects of the mask
    (``instances.detect_instances`` of the mask probability at ``threshold`` with ``min_area``, ``fill_holes``, ``connectivity``):
    "instances" (per image the records: id, area, box, centroid, score), "instance_labels" int32 [N, H, W], "clean_mask" bool
    [N, H, W] (the mask without its small components, with its holes filled) and "instance_counts" int32 [N, 4]; with ``gt_masks``
    also "clean_metrics", ``segmentation_metrics`` of the clean mask.  "metrics" and "cod_metrics" score the raw probability either way.
    ``refine`` -- ``None`` (off: no launch more than before), ``True`` or a dict with any of "radius" (8), "eps" (1e-4), "guide" ("rgb",
    or "gray": the luma 0.2989 r + 0.5870 g + 0.1140 b of the image, taken in fp32 on the device) -- snaps the mask probability to
    the image's edges with ``refine.guided_filter`` (include/camo_guided.h) and adds "prob_refined" fp32 [N, H, W] (clamped to
    [0, 1]), "mask_refined" bool [N, H, W] (> ``threshold``) and "refine_coefficients" fp32 [N, C + 1, H, W] (what
    ``refine.guided_upsample`` takes to a native size); with ``gt_masks`` also "refined_metrics" and, with ``cod_metrics=True``,
    "refined_cod_metrics".  Every other key keeps its bytes; the instances of the refined map are
    ``detect_instances(out["prob_refined"], ...)``.
    ``match`` -- ``None`` (off: no launch more than before), ``True`` or a dict with any of "thresholds" (COCO's 0.50 .. 0.95),
    "gt_labels" (int32 [N, H, W] ground-truth ids; default: the connected components of ``gt_masks`` with ``connectivity``) and
    "max_gt" (64) -- needs ``instances=True`` and ``gt_masks`` or "gt_labels"; it matches the instances to the ground-truth ones
    (``instance_match.match_detected``, include/camo_inst_match.h) and adds "instance_match" (per image the records of
    ``instance_match_records``) and "instance_match_tables" (``match_instances``' dict).  Every other key keeps its bytes.
    "gt_rles" in ``match`` -- per image a list of COCO RLE dicts or (rle, id) pairs -- gives the ground-truth ids in the place of
    "gt_labels" (both together raise): ``rle.decode_rles`` paints them on the device (include/camo_rle.h).
    "gt_segmentations" in ``match`` -- per image a list of COCO ``segmentation`` fields, polygon lists or RLE dicts, or
    (segmentation, id) pairs -- does the same for annotations as a COCO file holds them (``polygons.decode_segmentations``,
    include/camo_poly.h); it goes with neither of the other two.
    ``rle=True`` (needs ``instances=True``) adds "instance_rles": per image {id: {"size": [H, W], "counts": str}}, the COCO run-length
    encoding of every instance of "instance_labels" (``rle.encode_instances``); ``False``: no launch more than before.
    ``boundary`` -- ``None`` (off: no launch more than before), ``True`` or a dict with any of "ratio" (1/50 of the diagonal) and
    "distance" (the erosion distance itself) -- needs ``match``; it matches the instances once more under min(mask IoU, boundary IoU)
    (``boundary.match_detected_boundary``, include/camo_boundary.h) and adds "boundary_match" (per image the records of
    ``boundary.boundary_match_records``: ``InstanceAP`` of them is Boundary AP) and "boundary_match_tables"; with ``gt_masks`` also
    "boundary_iou" (per image ``boundary.boundary_iou`` of "mask" against the ground-truth mask) and, with ``refine``,
    "refined_boundary_iou" (of "mask_refined": what the guided filter did to the contour).  Every other key keeps its bytes.
    ``split`` -- ``False`` (off: no launch more than before), ``True`` or a dict with any of "ratio" ((7, 10)), "min_core" (0),
    "max_split" (4), "max_instances" (64), "growth" ("euclidean"; "geodesic": connected parts, include/camo_split_geo.h, at the
    cost of one host synchronisation) and "rounds" -- needs ``instances=True``; it splits the touching objects of "instance_labels" at their
    necks (``split.split_detected``, include/camo_split.h) and adds "split_instances" (per image the records of
    ``split.split_records``, scored by the mask probability), "split_labels" int32 [N, H, W] and "split_counts" int32 [N, 4].
    ``match``, ``boundary`` and ``rle`` then work on the split labels and table, so instance AP and Boundary AP measure the split;
    "instances", "instance_labels", "clean_mask" and every metric of the mask keep their bytes.  "merge" in ``split`` -- a pair
    (num, den), e.g. (4, 5) -- joins the parts across their high passes after the split (``split.merge_parts``,
    include/camo_split_merge.h): "split_instances" and "split_labels" are then the merged ones, "split_counts" stays the splitter's,
    and the one key more is "split_merge_counts" int32 [N, 4].
    ``polygons=True`` (needs ``instances=True``) adds "instance_polygons": per image {id: {"polygons": [[x0, y0, x1, y1, ...], ...],
    "holes": [...], "area": pixels}}, the outlines of every instance of the labels ``rle`` works on, vertices on pixel corners, traced
    with the call's ``connectivity`` (``contours.encode_instance_polygons``, include/camo_contours.h); a polygon list is a union, so
    painting "polygons" back rebuilds an instance with its holes filled -- exact with ``fill_holes=True``, and "holes" carries what to
    subtract without it.  ``False``: no launch more than before."""
    if instances:
        _instances.check_arguments(threshold, connectivity, min_area)
    rle = _rle.rle_options(rle, instances)
    polygons = _contours.contour_options(polygons, instances)
    split = _split.split_options(split, instances)
    match = _match.match_options(match, instances, gt_masks is not None)
    boundary = _boundary.boundary_options(boundary, match)
    refine = _refine.refine_options(refine)
    img, _ = _image_batch(_as_tensor(images, device))
    _lib.require_device(img, "images")
    N, H, W = img.shape[:3]
    gt = None
    if gt_masks is not None:
        gt = gt_masks if isinstance(gt_masks, torch.Tensor) else torch.as_tensor(gt_masks)
        if tuple(gt.shape) != (N, H, W):
            raise ValueError(f"need gt_masks [N, H, W] = {(N, H, W)}, got {tuple(gt.shape)}")
        gt = gt.to(img.device)
    segments = slic_segments(img, n_segments)
    graphs, region_map = create_region_graphs_from_segments(img, segments, device=img.device, label_bound=slic_label_bound(H, W, n_segments))
    node_probs = rg_model.node_probabilities(graphs)
    prob_maps = paint_regions(node_probs, segments, region_map, graphs.node_offsets)
    out = {"prob_maps": prob_maps, "mask": prob_maps[:, 0] > threshold, "node_probs": node_probs, "graphs": graphs, "segments": segments,
           "region_map": region_map}
    if gt is not None:
        out["metrics"] = segmentation_metrics(segmentation_counts(prob_maps[:, 0], gt, threshold), H, W)
        if cod_metrics:
            out["cod_metrics"] = seg_measures.cod_metrics(prob_maps[:, 0], gt)
    elif cod_metrics:
        raise ValueError("cod_metrics=True needs gt_masks")
    if instances:
        found = _instances.detect_instances(prob_maps[:, 0], threshold, connectivity, min_area, fill_holes)
        out.update({"instances": found["instances"], "instance_labels": found["labels"], "clean_mask": found["clean_mask"],
                    "instance_counts": found["counts"]})
        if gt is not None:
            out["clean_metrics"] = segmentation_metrics(segmentation_counts(found["clean_mask"].float(), gt, 0.5), H, W)
        if split is not None:
            found = _split_found(found, prob_maps[:, 0], split)
            out.update({"split_instances": found["instances"], "split_labels": found["labels"], "split_counts": found["counts"]})
            if "merge" in split:
                out["split_merge_counts"] = found["merge_counts"]
        if match is not None:
            gt_labels = match["gt_labels"]      # (a [N, H, W] tensor goes on as it is: ``match_detected`` holds it to the labels' shape)
            if gt_labels is None:
                gt_labels = torch.stack(_match_ground_truth(match, N, "images", [(H, W)] * N, gt, connectivity, img.device))
            out["instance_match"], out["instance_match_tables"] = _match.match_detected(found["labels"], found["table"], gt_labels, match)
            if boundary is not None:
                out["boundary_match"], out["boundary_match_tables"] = _boundary.match_detected_boundary(found["labels"], found["table"], gt_labels,
                                                                                                        match, boundary)
        if rle:
            out["instance_rles"] = _rle.encode_instances(found["labels"])
        if polygons:
            out["instance_polygons"] = _contours.encode_instance_polygons(found["labels"], connectivity)
    if boundary is not None and gt is not None:
        out["boundary_iou"] = _boundary.boundary_iou(out["mask"], _positive(gt), boundary["distance"], boundary["ratio"])
    if refine is not None:
        guide = img if refine["guide"] == "rgb" else _refine.luma(img)
        q, coef = _refine.guided_filter(guide, prob_maps[:, 0], refine["radius"], refine["eps"], True, True)
        out.update({"prob_refined": q, "mask_refined": q > threshold, "refine_coefficients": coef})
        if gt is not None:
            out["refined_metrics"] = segmentation_metrics(segmentation_counts(q, gt, threshold), H, W)
            if cod_metrics:
                out["refined_cod_metrics"] = seg_measures.cod_metrics(q, gt)
            if boundary is not None:
                out["refined_boundary_iou"] = _boundary.boundary_iou(out["mask_refined"], _positive(gt), boundary["distance"], boundary["ratio"])
    return out


def detect_camouflage(rg_model, image, gt_mask=None, n_segments=500, threshold=0.5, device="cuda", cod_metrics=False, instances=False,
                      min_area=0, fill_holes=False, connectivity=8, refine=None, *, match=None, rle=False, boundary=None, split=False,
                      polygons=False):
    """The reference function's name: ``detect_camouflage_batch`` on one ``image`` [H, W, 3] (``gt_mask`` [H, W]); same dict."""
    img = image if isinstance(image, torch.Tensor) else torch.as_tensor(image).to(torch.device(device))
    if img.dim() != 3:
        raise ValueError(f"need image [H, W, 3], got {tuple(img.shape)}")
    gt = None if gt_mask is None else (gt_mask if isinstance(gt_mask, torch.Tensor) else torch.as_tensor(gt_mask)).unsqueeze(0)
    return detect_camouflage_batch(rg_model, img.unsqueeze(0), gt, n_segments, threshold, device, cod_metrics, instances, min_area, fill_holes,
                                   connectivity, refine, match=match, rle=rle, boundary=boundary, split=split, polygons=polygons)


@torch.no_grad()
def detect_camouflage_ragged(rg_model, images, gt_masks=None, size=(256, 256), n_segments=500, threshold=0.5, device="cuda",
                             cod_metrics=False, evaluate_at="native", instances=False, min_area=0, fill_holes=False, connectivity=8, refine=None,
                             *, match=None, rle=False, boundary=None, split=False, polygons=False):
    """``detect_camouflage_batch`` for uint8 images of mixed sizes (``resize_batch``'s ``images``): resized to ``size`` (bilinear) on
    the device, detected there, and the mask probability resized back to every image's own size (bilinear).  Returns
    ``detect_camouflage_batch``'s dict (everything at ``size``) plus "prob_maps_native": the list of fp32 [H_i, W_i] maps (views of
    one buffer) and "mask_native": the list of bool [H_i, W_i] (probability > ``threshold``).  With ``gt_masks`` (N masks [H_i, W_i],
    uint8 positive above 127, or bool) "metrics" -- and "cod_metrics" with ``cod_metrics=True`` -- are taken per image against its own
    mask at its own size, which is where the benchmark tables take them; images of equal size share a call.
    ``evaluate_at="resized"`` resizes the masks down (nearest) instead and scores at ``size``, as the reference does.
    ``instances=True`` takes the objects of every NATIVE-size map (``instances.detect_instances`` at ``threshold`` with ``min_area``,
    ``fill_holes``, ``connectivity``; maps of equal size share a call): "instances_native" (per image the records),
    "instance_labels_native" (int32 [H_i, W_i]) and "clean_mask_native" (bool [H_i, W_i]); with masks scored at native size also
    "clean_metrics", ``segmentation_metrics`` of every clean mask against its own mask.
    ``refine`` (``detect_camouflage_batch``'s; the guide must be "rgb") runs the guided filter at ``size`` on the resized image and
    applies its coefficients to the NATIVE bytes of every image (``refine.guided_upsample``: the fast guided filter), so the native
    map's edges come from the native pixels: "prob_maps_native_refined" (fp32 [H_i, W_i], views of one buffer) and
    "mask_native_refined" beside ``detect_camouflage_batch``'s own refine keys at ``size``; with masks scored at native size also
    "refined_metrics" / "refined_cod_metrics" of the native refined maps.  "prob_maps_native" and the rest are unchanged.
    ``match`` (``detect_camouflage_batch``'s; "gt_labels" is a list of int32 [H_i, W_i] maps) matches the NATIVE-size instances to
    the ground-truth ones -- by default the connected components of every native mask, which needs ``gt_masks`` scored at native
    size; images of equal size share a call -- and adds "instance_match" (per image the records) and "instance_match_tables" (per
    image ``match_instances``' dict of its own rows).  ``None``: nothing changes.  "gt_rles" in ``match`` holds per image the COCO RLEs of
    its ground-truth instances at the image's NATIVE size (``rle.decode_rles``; images of equal size share a call);
    "gt_segmentations" holds per image its COCO ``segmentation`` fields, polygons or RLEs, in NATIVE coordinates
    (``polygons.decode_segmentations``; images of equal size share a call).
    ``rle=True`` (needs ``instances=True``) adds "instance_rles_native": per image {id: RLE} of "instance_labels_native"
    (``rle.encode_instances``; maps of equal size share a call).
    ``boundary`` (``detect_camouflage_batch``'s; needs ``match``) works at NATIVE size, with the distance of every size group from
    its own H and W: "boundary_match" (per image the records), "boundary_match_tables" (per image its own rows) and, with masks
    scored at native size, "boundary_iou" of "mask_native" and, with ``refine``, "refined_boundary_iou" of "mask_native_refined".
    ``split`` (``detect_camouflage_batch``'s; needs ``instances=True``) splits the NATIVE-size instances, maps of equal size sharing a
    call: "split_instances_native" (per image the records), "split_labels_native" (int32 [H_i, W_i]) and "split_counts_native"
    (int32 [4]); ``match``, ``boundary`` and ``rle`` then work on them.  With "merge" in ``split`` they are the merged ones, and
    "split_merge_counts_native" (int32 [4] per image) is the one key more.
    ``polygons=True`` (needs ``instances=True``) adds "instance_polygons_native": per image {id: {"polygons", "holes", "area"}} of the
    labels ``rle`` works on, in NATIVE coordinates (``contours.encode_instance_polygons`` with ``connectivity``; maps of equal size
    share a call); painting "polygons" back rebuilds an instance with its holes filled, so the round trip is exact with
    ``fill_holes=True`` and "holes" carries what to subtract without it."""
    if instances:
        _instances.check_arguments(threshold, connectivity, min_area)
    rle = _rle.rle_options(rle, instances)
    polygons = _contours.contour_options(polygons, instances)
    split = _split.split_options(split, instances)
    match = _match.match_options(match, instances, gt_masks is not None and evaluate_at == "native")
    boundary = _boundary.boundary_options(boundary, match)
    refine = _refine.refine_options(refine)
    if refine is not None and refine["guide"] != "rgb":
        raise ValueError('detect_camouflage_ragged applies the coefficients to the native 3-channel bytes: refine["guide"] must be "rgb"')
    if evaluate_at not in ("native", "resized"):
        raise ValueError(f'evaluate_at must be "native" or "resized", got {evaluate_at!r}')
    if cod_metrics and gt_masks is None:
        raise ValueError("cod_metrics=True needs gt_masks")
    data, geo, C, squeeze = _ragged(images, device)
    if C != 3:
        raise ValueError(f"need images with 3 channels, got {C}")
    packed = _packed(data, geo, C)
    sizes = packed.sizes
    img = resize_batch(packed, size, "bilinear")
    masks = None if gt_masks is None else _mask_list(gt_masks, len(sizes), "gt_masks", img.device)
    if masks is not None and evaluate_at == "native" and masks.sizes != sizes:
        raise ValueError("every ground-truth mask must have its image's size")
    resized = masks is not None and evaluate_at == "resized"
    gt = resize_batch(masks, size, "nearest", out_dtype=torch.uint8) if resized else None
    truth = [masks.image(i) for i in range(len(sizes))] if masks is not None and not resized else None      # (the masks to score against)
    out = detect_camouflage_batch(rg_model, img, gt, n_segments, threshold, img.device, cod_metrics and resized, refine=refine)
    native, _ = resize_to_sizes(out["prob_maps"][:, 0], sizes, "bilinear")
    out["prob_maps_native"] = native
    out["mask_native"] = [p > threshold for p in native]
    if truth is not None:
        out["metrics"], cods = _score(native, truth, threshold, cod_metrics)
        if cod_metrics:
            out["cod_metrics"] = cods
    if instances:
        def found(idx, _):
            f = _instances.detect_instances(_stack(native, idx), threshold, connectivity, min_area, fill_holes)
            return f["instances"], f["labels"], f["clean_mask"], f["table"]

        rec, labels, clean, tables = _by_size(native, found, 4)
        out.update({"instances_native": rec, "instance_labels_native": labels, "clean_mask_native": clean})
        if truth is not None:
            out["clean_metrics"], _ = _score([c.float() for c in clean], truth, 0.5, False)
        if split is not None:
            def parts(idx, _):
                f = _split_found({"instances": [rec[i] for i in idx], "labels": _stack(labels, idx)}, _stack(native, idx), split)
                return f["instances"], f["labels"], f["table"], f["counts"], f.get("merge_counts", [None] * len(idx))

            split_rec, labels, tables, split_counts, merge_counts = _by_size(native, parts, 5)
            out.update({"split_instances_native": split_rec, "split_labels_native": labels, "split_counts_native": split_counts})
            if "merge" in split:
                out["split_merge_counts_native"] = merge_counts
        if match is not None:
            gt_labels = _match_ground_truth(match, len(sizes), "images", sizes, truth, connectivity, img.device)
            out["instance_match"], out["instance_match_tables"] = _native_matches(labels, tables, gt_labels, match)
            if boundary is not None:
                out["boundary_match"], out["boundary_match_tables"] = _native_boundary_matches(labels, tables, gt_labels, match, boundary)
        if rle:
            out["instance_rles_native"] = _by_size(labels, lambda idx, _: _rle.encode_instances(_stack(labels, idx)))
        if polygons:
            out["instance_polygons_native"] = _by_size(labels, lambda idx, _: _contours.encode_instance_polygons(_stack(labels, idx), connectivity))
    if boundary is not None and truth is not None:
        out["boundary_iou"] = _native_boundary_ious(out["mask_native"], truth, boundary)
    if refine is not None:
        refined, _ = _refine.guided_upsample(out["refine_coefficients"], packed)
        out["prob_maps_native_refined"] = refined
        out["mask_native_refined"] = [p > threshold for p in refined]
        if truth is not None:
            out["refined_metrics"], cods = _score(refined, truth, threshold, cod_metrics)
            if cod_metrics:
                out["refined_cod_metrics"] = cods
            if boundary is not None:
                out["refined_boundary_iou"] = _native_boundary_ious(out["mask_native_refined"], truth, boundary)
    return out


def quantise_map(pred):
    """The 8-bit value of include/camo_seg_measures.h of every element: rint(clamp(pred, 0, 1) * 255) with the multiply in fp32, ties
    to even, a NaN gives 0 -> uint8."""
    p = pred.to(torch.float32)
    p = torch.where(p != p, torch.zeros_like(p), p).clamp(0.0, 1.0)
    return (p * 255.0).round().to(torch.uint8)


def _files_by_stem(folder):
    return {os.path.splitext(f)[0]: os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.lower().endswith(IMAGE_SUFFIXES)}


def detect_camouflage_directory(rg_model, image_dir, mask_dir=None, out_dir=None, batch_size=16, results_json=None, image_ids=None,
                                annotations_json=None, **kw):
    """``detect_camouflage_ragged`` over the image files of ``image_dir`` (read with PIL, in sorted order, ``batch_size`` at a time;
    ``**kw`` goes to it).  With ``mask_dir`` every image needs a mask file of the same stem.  With ``out_dir`` every native-size mask
    probability is written there as ``<stem>.png``, 8 bits, quantised as include/camo_seg_measures.h quantises (``quantise_map``).
    Returns {"files": stems, "metrics": per-file ``segmentation_metrics`` dicts and, with ``cod_metrics=True``, "cod_metrics":
    per-file measures and "aggregate": ``seg_measures.aggregate_cod_measures`` of them}; the last three only with masks.
    With ``refine`` (``detect_camouflage_ragged``'s) the map written to ``out_dir`` and the map scored are the REFINED ones
    ("prob_maps_native_refined"; "prob_refined" with ``evaluate_at="resized"``); without it nothing changes.
    With ``match`` (``detect_camouflage_ragged``'s; needs ``instances=True`` and ``mask_dir``, or "gt_labels" for every file in
    sorted order) the native-size instances of every file are matched to the ground-truth ones and the result also holds
    "instance_match" (per-file records) and "instance_ap": ``instance_match.InstanceAP`` over all files, scored by every instance's
    mean probability.  "gt_rles" in ``match`` holds the RLE lists of every file in sorted order, as "gt_labels" does, and
    "gt_segmentations" the lists of COCO ``segmentation`` fields.  "gt_coco" in ``match`` -- the path of a COCO annotations file, or its
    dict -- takes them from that file by file stem (``polygons.coco_ground_truth``; a file whose size is not the one the annotations
    state raises) and, with ``results_json`` and no ``image_ids``, numbers the results with the file's image ids.
    ``results_json`` (a path; needs ``instances=True``) writes the native-size instances of every file as a COCO results list: per
    instance {"image_id": the stem, or ``image_ids[stem]``, "category_id": 1, "segmentation": {"size", "counts"} (include/camo_rle.h),
    "score": the instance's Sq / (255 area), "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1]}; the result also holds "results": that list.
    With ``boundary`` (``detect_camouflage_ragged``'s; needs ``match``) the result also holds "boundary_match" (per-file records) and
    "boundary_ap": ``InstanceAP`` over them, which is Boundary AP; with masks scored at native size also "boundary_iou" per file and,
    with ``refine``, "refined_boundary_iou".
    With ``split`` (``detect_camouflage_ragged``'s; needs ``instances=True``) the instances matched, scored and written to
    ``results_json`` are the split ones ("split_instances_native"), the merged ones with "merge" in ``split``.
    ``annotations_json`` (a path; needs ``instances=True``, sets ``polygons=True``) writes the same instances as a COCO annotations
    file {"images", "annotations", "categories": [{"id": 1, "name": "camouflaged"}]} with native-size polygons
    (``contours.coco_annotations``): what ``polygons.coco_ground_truth`` and "gt_coco" read, so the detector's proposals can be
    corrected in an annotation tool and fine-tuned from.  ``image_ids`` applies as for ``results_json``, and the two files may be asked
    for together; the result also holds "annotations": the file's dict.  A polygon list is a union, so a reader rebuilds every instance
    with its holes filled: the round trip is exact with ``fill_holes=True``, and "holes" carries what to subtract without it."""
    from PIL import Image
    refined = _refine.refine_options(kw.get("refine")) is not None
    found_key = "instances_native" if _split.split_options(kw.get("split", False), kw.get("instances", False)) is None else "split_instances_native"
    match = _match.match_options(kw.pop("match", None), kw.get("instances", False), mask_dir is not None, coco=True)
    boundary = _boundary.boundary_options(kw.get("boundary"), match)
    if results_json is not None:
        if not isinstance(results_json, (str, os.PathLike)):
            raise ValueError(f"results_json must be a path, got {results_json!r}")
        if not kw.get("instances", False):
            raise ValueError("results_json needs instances=True: the instances are what it writes")
        kw["rle"] = True
    if annotations_json is not None:
        if not isinstance(annotations_json, (str, os.PathLike)):
            raise ValueError(f"annotations_json must be a path, got {annotations_json!r}")
        if not kw.get("instances", False):
            raise ValueError("annotations_json needs instances=True: the instances are what it writes")
        kw["polygons"] = True
    if image_ids is not None and results_json is None and annotations_json is None:
        raise ValueError("image_ids needs results_json or annotations_json")
    if image_ids is not None and not isinstance(image_ids, dict):
        raise ValueError(f"image_ids must be a dict from file stem to image id, got {type(image_ids).__name__}")
    cod = bool(kw.pop("cod_metrics", False))
    evaluate_at = kw.pop("evaluate_at", "native")
    threshold = kw.get("threshold", 0.5)
    size = kw.get("size", (256, 256))
    images = _files_by_stem(image_dir)
    if not images:
        raise ValueError(f"no image file in {image_dir}")
    masks = None if mask_dir is None else _files_by_stem(mask_dir)
    if masks is not None and set(images) - set(masks):
        raise ValueError(f"no mask in {mask_dir} for {sorted(set(images) - set(masks))[:5]}")
    if cod and masks is None:
        raise ValueError("cod_metrics=True needs mask_dir")
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    stems = list(images)
    result = {"files": stems}
    metrics, cods = [], []
    matched, ap = [], _match.InstanceAP()
    bd_matched, bd_ap, bd_ious, bd_refined = [], _match.InstanceAP(), [], []
    coco_sizes = source = None
    if match is not None:
        coco = match.pop("gt_coco")
        if coco is not None:
            truth = _polygons.coco_ground_truth(coco, stems)
            match["gt_segmentations"], coco_sizes = truth["segmentations"], truth["sizes"]
            if (results_json is not None or annotations_json is not None) and image_ids is None:
                image_ids = truth["image_ids"]
        _check_sources(match, len(stems), "files")      # (for the whole directory, before any file is read)
        source = next((key for key, _ in GT_SOURCES if match[key] is not None), None)
    if image_ids is not None and set(stems) - set(image_ids):
        raise ValueError(f"image_ids has no entry for {sorted(set(stems) - set(image_ids))[:5]}")
    results, coco_images, coco_anns = [], [], []
    for at in range(0, len(stems), int(batch_size)):
        part = stems[at:at + int(batch_size)]
        arrays = [np.array(Image.open(images[s]).convert("RGB")) for s in part]
        gts = None
        if masks is not None:
            gts = _mask_list([np.array(Image.open(masks[s]).convert("L")) for s in part], len(part), "masks", _device(kw.get("device", "cuda")))
        if coco_sizes is not None:
            for s, a, size in zip(part, arrays, coco_sizes[at:at + len(part)]):
                if tuple(a.shape[:2]) != tuple(size):
                    raise ValueError(f"{s} is {a.shape[0]} x {a.shape[1]} and the annotations state {size[0]} x {size[1]}")
        if match is None:
            out = detect_camouflage_ragged(rg_model, arrays, **kw)
        else:                                            # (this batch's slice of the one source; without one, the components of its masks)
            ids = match[source][at:at + len(part)] if source is not None else \
                _match_ground_truth(match, len(part), "files", gts.sizes, [gts.image(i) for i in range(len(part))], kw.get("connectivity", 8), None)
            out = detect_camouflage_ragged(rg_model, arrays, match=dict(match, **{source or "gt_labels": ids}), **kw)
            matched += out["instance_match"]
            scores = [[inst["score"] for inst in r["instances"]] for r in out[found_key]]
            ap.add(out["instance_match"], scores)
            if boundary is not None:
                bd_matched += out["boundary_match"]
                bd_ap.add(out["boundary_match"], scores)
        if results_json is not None:
            results += _rle.coco_results(part, out[found_key], out["instance_rles_native"], image_ids)
        if annotations_json is not None:
            ims, anns = _contours.coco_annotations(part, [a.shape[:2] for a in arrays], out[found_key], out["instance_polygons_native"], image_ids)
            coco_images += ims
            coco_anns += [dict(a, id=len(coco_anns) + k + 1) for k, a in enumerate(anns)]      # (numbered over the whole directory)
        native = out["prob_maps_native_refined" if refined else "prob_maps_native"]
        if out_dir is not None:
            for s, p in zip(part, native):
                Image.fromarray(quantise_map(p).cpu().numpy()).save(os.path.join(out_dir, s + ".png"))
        if masks is not None:
            if evaluate_at == "resized":
                small = resize_batch(gts, size, "nearest", out_dtype=torch.uint8)
                m, c = _score(list(out["prob_refined"] if refined else out["prob_maps"][:, 0]), list(small), threshold, cod, curves=True)
            else:
                truth = [gts.image(i) for i in range(len(part))]
                m, c = _score(native, truth, threshold, cod, curves=True)
                if boundary is not None:                 # (the ragged call above was given no masks: the files' masks are scored here)
                    bd_ious += _native_boundary_ious(out["mask_native"], truth, boundary)
                    if refined:
                        bd_refined += _native_boundary_ious(out["mask_native_refined"], truth, boundary)
            metrics += m
            cods += c or []
    if masks is not None:
        result["metrics"] = metrics
        if cod:
            result["aggregate"] = seg_measures.aggregate_cod_measures(cods)
            result["cod_metrics"] = [{k: v for k, v in c.items() if k not in ("f_curve", "e_curve")} for c in cods]
    if match is not None:
        result["instance_match"], result["instance_ap"] = matched, ap.result()
    if boundary is not None:
        result["boundary_match"], result["boundary_ap"] = bd_matched, bd_ap.result()
        if masks is not None and evaluate_at == "native":
            result["boundary_iou"] = bd_ious
            if refined:
                result["refined_boundary_iou"] = bd_refined
    if results_json is not None:
        with open(results_json, "w") as f:
            json.dump(results, f)
        result["results"] = results
    if annotations_json is not None:
        result["annotations"] = {"images": coco_images, "annotations": coco_anns, "categories": [{"id": 1, "name": "camouflaged"}]}
        with open(annotations_json, "w") as f:
            json.dump(result["annotations"], f)
    return result
