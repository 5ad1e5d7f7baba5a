"""The region-graph detector on MI355X: where the object is (include/camo_rg_detect.h).

The kernels under the reference's ``detect_camouflage`` (models/region_graph/test.py) -- the only pixel mask and the only IoU /
Dice / precision / recall / F1 of the reference -- with nothing on the host: after the node-classification heads of
``RegionGraphGNN`` (region_graph.py, one launch) every probability is painted onto its superpixel's pixels in one launch
(``paint_regions``), and the painted mask is counted against a ground-truth mask in two (``segmentation_counts``).  This module is
the header's binding; ``detect_camouflage_batch`` and ``detect_camouflage``, which put these calls together, are in pipeline.py.
PARITY UNPINNED: the reference tree, torch_geometric, scikit-image and an RG checkpoint are absent, so the header's text is the
definition.  There is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, image_planes


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
    call("camo_rg_paint", dev, _ptr(val), n, ch, _ptr(seg), _ptr(rmap), _ptr(off), N, H, W, rmap.shape[1], float(fill), _ptr(maps), _stream_ptr(dev))
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
    pred, stride = image_planes(pred)
    dev = pred.device
    g = gt.to(device=dev)
    g = (g.to(torch.uint8) * 255 if g.dtype == torch.bool else g.to(torch.uint8)).contiguous()
    counts = torch.empty(N, 5, dtype=torch.int64, device=dev)
    call("camo_seg_counts", dev, _ptr(pred), stride, _ptr(g), float(threshold), N, H, W, _ptr(counts), _stream_ptr(dev))
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
