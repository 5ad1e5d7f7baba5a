"""The region-graph detector on MI355X: where the object is (include/camo_rg_detect.h).

The reference's ``detect_camouflage`` (models/region_graph/test.py) -- the only pixel mask and the only IoU / Dice / precision /
recall / F1 of the reference -- for a batch of images with nothing on the host: superpixels, edge maps and region graphs on the
device (region_graph.py), the node-classification heads of ``RegionGraphGNN`` in one launch, every probability painted onto its
superpixel's pixels in one launch, and the painted mask counted against a ground-truth mask in two.  PARITY UNPINNED: the
reference tree, torch_geometric, scikit-image and an RG checkpoint are absent, so the header's text is the definition.  There
is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import torch

from . import _lib, instance_match as _match, instances as _instances, polygons as _polygons, refine as _refine, rle as _rle, seg_measures
from .engine import _ptr, _stream_ptr
from .region_graph import _as_tensor, _image_batch, create_region_graphs_from_segments, slic_label_bound, slic_segments


def _offsets_tensor(node_offsets, device):
    if isinstance(node_offsets, torch.Tensor):
        return node_offsets.to(device=device, dtype=torch.int32).contiguous()
    return torch.tensor(list(node_offsets), dtype=torch.int32, device=device)


@torch.no_grad()
def paint_regions(values, segments, region_map, node_offsets, fill=0.0):
    """A value per region onto the region's pixels (``camo_rg_paint``): ``values`` [n, C] (or [n]) rows of the block-diagonal graph,
    ``segments`` [N, H, W] integer labels, ``region_map`` [N, label_bound] and ``node_offsets`` (N + 1 integers, list or tensor) as
    ``create_region_graphs_from_segments`` returns them -> fp32 [N, C, H, W]; a pixel whose label has no region gets ``fill``.
    A single image -- ``segments`` [H, W] with ``region_map`` [labels]; ``node_offsets`` may be ``None`` -- is N = 1.  Bit-exact."""
    _lib.require_device(values, "values")
    _lib.require_device(segments, "segments")
    _lib.require_device(region_map, "region_map")
    dev = values.device
    val = values.detach().to(torch.float32)
    if val.dim() == 1:
        val = val.unsqueeze(1)
    if segments.dim() == 2:
        segments, region_map = segments.unsqueeze(0), region_map.reshape(1, -1)
        if node_offsets is None:
            node_offsets = [0, val.shape[0]]
    if val.dim() != 2 or segments.dim() != 3 or region_map.dim() != 2 or region_map.shape[0] != segments.shape[0] or val.numel() == 0 \
            or segments.numel() == 0 or region_map.numel() == 0:
        raise ValueError(f"need values [n, C], segments [N, H, W], region_map [N, label_bound]; got {tuple(values.shape)}, "
                         f"{tuple(segments.shape)}, {tuple(region_map.shape)}")
    n, ch = val.shape
    if ch > _lib.RGD_MAX_CHANNELS:
        raise ValueError(f"at most {_lib.RGD_MAX_CHANNELS} channels, got {ch}")
    N, H, W = segments.shape
    off = _offsets_tensor(node_offsets, dev)
    if off.numel() != N + 1:
        raise ValueError(f"node_offsets must hold N + 1 = {N + 1} integers, got {off.numel()}")
    val = val.contiguous()
    seg = segments.to(device=dev, dtype=torch.int32).contiguous()
    rmap = region_map.to(device=dev, dtype=torch.int32).contiguous()
    maps = torch.empty(N, ch, H, W, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().camo_rg_paint(_ptr(val), n, ch, _ptr(seg), _ptr(rmap), _ptr(off), N, H, W, rmap.shape[1], float(fill), _ptr(maps),
                                      _stream_ptr(dev))
    _lib.check(rc, "camo_rg_paint")
    return maps


@torch.no_grad()
def attention_to_pixels(attn_list, segments, region_map, node_offsets):
    """The fusion model's knowledge-graph -> region attention as per-pixel heat maps: ``attn_list`` holds per image either the
    ``kg2rg`` map [Nk, Nr_i] or the dict ``predict_batch_from_images`` returns (its ``"kg2rg"`` is used); the maps are transposed
    and stacked to [n, Nk] and painted -> [N, Nk, H, W] (Nk <= 16)."""
    rows = [(a["kg2rg"] if isinstance(a, dict) else a) for a in attn_list]
    if not rows:
        raise ValueError("attention_to_pixels needs at least one image")
    for a in rows:
        _lib.require_device(a, "attention maps")
    return paint_regions(torch.cat([a.detach().to(torch.float32).reshape(a.shape[-2], a.shape[-1]).t() for a in rows]), segments,
                         region_map, node_offsets)


@torch.no_grad()
def segmentation_counts(pred, gt, threshold=0.5):
    """A predicted map against a ground-truth mask (``camo_seg_counts``): ``pred`` fp32 [N, H, W] (or [H, W]; one channel of a
    [N, C, H, W] map is read in place), ``gt`` [N, H, W] uint8 (positive above 127) or bool -> int64 [N, 5] on the device =
    TP, FP, FN, TN, A with A = sum of llrint(|pred - g| 2^32).  Integer sums: two calls give the same bytes."""
    _lib.require_device(pred, "pred")
    _lib.require_device(gt, "gt")
    if pred.dim() == 2:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
    if pred.dim() != 3 or gt.shape != pred.shape or pred.numel() == 0:
        raise ValueError(f"need pred [N, H, W] and gt of the same shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    N, H, W = pred.shape
    pred = pred.detach()
    if pred.dtype != torch.float32 or pred.stride(2) != 1 or pred.stride(1) != W or (N > 1 and pred.stride(0) < H * W):
        pred = pred.to(torch.float32).contiguous()
    stride = pred.stride(0) if N > 1 else H * W
    dev = pred.device
    g = gt.to(device=dev)
    g = (g.to(torch.uint8) * 255 if g.dtype == torch.bool else g.to(torch.uint8)).contiguous()
    counts = torch.empty(N, 5, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().camo_seg_counts(_ptr(pred), stride, _ptr(g), float(threshold), N, H, W, _ptr(counts), _stream_ptr(dev))
    _lib.check(rc, "camo_seg_counts")
    return counts


def segmentation_metrics(counts, H, W):
    """The ratios of include/camo_rg_detect.h from ``segmentation_counts``' [N, 5] (tensor or nested list), on the host in float64:
    a list of dicts with iou, dice, precision, recall, f1, accuracy, mae and the four counts.  IoU and Dice are 1 when both masks
    are empty; precision, recall and F1 are 0 when their denominator is 0."""
    rows = counts.tolist() if isinstance(counts, torch.Tensor) else [list(r) for r in counts]      # (a device tensor: the one copy)
    hw = float(H) * float(W)
    out = []
    for tp, fp, fn, tn, a in rows:
        tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
        p = tp / (tp + fp) if tp + fp else 0.0
        r = tp / (tp + fn) if tp + fn else 0.0
        out.append({"iou": tp / (tp + fp + fn) if tp + fp + fn else 1.0,
                    "dice": 2 * tp / (2 * tp + fp + fn) if tp + fp + fn else 1.0,
                    "precision": p, "recall": r, "f1": 2 * p * r / (p + r) if p + r else 0.0,
                    "accuracy": (tp + tn) / hw, "mae": int(a) / 2.0 ** _lib.RGD_FIX_BITS / hw,
                    "tp": tp, "fp": fp, "fn": fn, "tn": tn})
    return out


@torch.no_grad()
def detect_camouflage_batch(rg_model, images, gt_masks=None, n_segments=500, threshold=0.5, device="cuda", cod_metrics=False,
                            instances=False, min_area=0, fill_holes=False, connectivity=8, refine=None, *, match=None, rle=False):
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
    encoding of every instance of "instance_labels" (``rle.encode_instances``); ``False``: no launch more than before."""
    if instances:
        _instances.check_arguments(threshold, connectivity, min_area)
    rle = _rle.rle_options(rle, instances)
    match = _match.match_options(match, instances, gt_masks is not None)
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
        if match is not None:
            if match["gt_rles"] is not None:
                if len(match["gt_rles"]) != N:
                    raise ValueError(f'match["gt_rles"] holds {len(match["gt_rles"])} lists for {N} images')
                gt_labels = _rle.decode_rles(match["gt_rles"], H, W, img.device)
            elif match["gt_segmentations"] is not None:
                if len(match["gt_segmentations"]) != N:
                    raise ValueError(f'match["gt_segmentations"] holds {len(match["gt_segmentations"])} lists for {N} images')
                gt_labels = _polygons.decode_segmentations(match["gt_segmentations"], H, W, img.device)
            else:
                gt_labels = match["gt_labels"] if match["gt_labels"] is not None else _match.ground_truth_labels(gt, connectivity, match["max_gt"])
            out["instance_match"], out["instance_match_tables"] = _match.match_detected(found["labels"], found["table"], gt_labels, match)
        if rle:
            out["instance_rles"] = _rle.encode_instances(found["labels"])
    if refine is not None:
        guide = img if refine["guide"] == "rgb" else _refine.luma(img)
        q, coef = _refine.guided_filter(guide, prob_maps[:, 0], refine["radius"], refine["eps"], True, True)
        out.update({"prob_refined": q, "mask_refined": q > threshold, "refine_coefficients": coef})
        if gt is not None:
            out["refined_metrics"] = segmentation_metrics(segmentation_counts(q, gt, threshold), H, W)
            if cod_metrics:
                out["refined_cod_metrics"] = seg_measures.cod_metrics(q, gt)
    return out


def detect_camouflage(rg_model, image, gt_mask=None, n_segments=500, threshold=0.5, device="cuda", cod_metrics=False, instances=False,
                      min_area=0, fill_holes=False, connectivity=8, refine=None, *, match=None, rle=False):
    """The reference function's name: ``detect_camouflage_batch`` on one ``image`` [H, W, 3] (``gt_mask`` [H, W]); same dict."""
    img = image if isinstance(image, torch.Tensor) else torch.as_tensor(image).to(torch.device(device))
    if img.dim() != 3:
        raise ValueError(f"need image [H, W, 3], got {tuple(img.shape)}")
    gt = None if gt_mask is None else (gt_mask if isinstance(gt_mask, torch.Tensor) else torch.as_tensor(gt_mask)).unsqueeze(0)
    return detect_camouflage_batch(rg_model, img.unsqueeze(0), gt, n_segments, threshold, device, cod_metrics, instances, min_area, fill_holes,
                                   connectivity, refine, match=match, rle=rle)
