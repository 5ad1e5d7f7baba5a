"""Object instances of a predicted mask on MI355X (include/camo_instances.h): how many objects a mask holds, each
one's box, size, centre and confidence, and the mask without specks and pinholes.

``mask_instances`` runs ``camo_instances`` -- binarise, fill holes, label the connected components, drop the small ones, number the
rest in reading order, sum an integer table per component -- and returns device tensors; ``instance_records`` takes the ratios from
the integers on the host in float64; ``detect_instances`` is the two together with a table that always holds every instance.
PARITY UNPINNED: the header's text is the definition (restated in numpy in tests/instances_ref.py).  There is no CPU path: tensors
that are not on a HIP device raise.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, image_planes, workspace


def check_arguments(threshold=0.5, connectivity=8, min_area=0, max_instances=64, n_images=1):
    """The ``ValueError`` of every bad setting, by name, before anything touches the device."""
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not math.isfinite(threshold):
        raise ValueError(f"threshold must be a finite number, got {threshold!r}")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, numbers.Integral) or min_area < 0:
        raise ValueError(f"min_area must be an integer >= 0, got {min_area!r}")
    if isinstance(max_instances, bool) or not isinstance(max_instances, numbers.Integral) or max_instances < 1:
        raise ValueError(f"max_instances must be an integer >= 1, got {max_instances!r}")
    if n_images * max_instances > _lib.INST_MAX_ROWS:
        raise ValueError(f"max_instances = {max_instances} for {n_images} images exceeds {_lib.INST_MAX_ROWS} table rows")


@torch.no_grad()
def mask_instances(pred, threshold=0.5, connectivity=8, min_area=0, fill_holes=False, max_instances=64):
    """``camo_instances``: ``pred`` fp32 [N, H, W] (or [H, W]; one channel of a [N, C, H, W] map is read in place) ->
    {"labels": int32 [N, H, W] (0 on background, ids 1 .. K in the reading order of every component's first pixel),
    "clean_mask": bool [N, H, W] (labels > 0), "table": int64 [N, max_instances, 8] = (area, x0, y0, x1, y1, Sx, Sy, Sq) of ids
    1 .. max_instances (zero past K), "counts": int32 [N, 4] = (K, components dropped as smaller than ``min_area``, holes filled,
    pixels of the clean mask)}, all on the device, no host synchronisation.  A pixel is foreground when ``pred > threshold``;
    ``fill_holes`` makes every background component that does not touch the image's border foreground first (background connectivity:
    the complement of ``connectivity``).  Integer sums and smallest-index roots: two calls give the same bytes."""
    if pred.dim() == 2:
        pred = pred.unsqueeze(0)
    if pred.dim() != 3 or pred.numel() == 0:
        raise ValueError(f"need pred [N, H, W] or [H, W] with at least one pixel, got {tuple(pred.shape)}")
    N, H, W = pred.shape
    check_arguments(threshold, connectivity, min_area, max_instances, N)
    _lib.require_device(pred, "pred")
    pred, stride = image_planes(pred)
    dev = pred.device
    ws, nbytes = workspace("camo_instances_workspace_bytes", N, H, W, device=dev,
                           refuse=lambda: ValueError(f"camo_instances does not support N = {N}, H = {H}, W = {W}"))
    labels = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    clean = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    table = torch.empty(N, int(max_instances), _lib.INST_FIELDS, dtype=torch.int64, device=dev)
    counts = torch.empty(N, _lib.INST_COUNTS, dtype=torch.int32, device=dev)
    call("camo_instances", dev, _ptr(pred), stride, float(threshold), N, H, W, int(connectivity), int(min_area), 1 if fill_holes else 0,
         int(max_instances), _ptr(labels), _ptr(clean), _ptr(table), _ptr(counts), _ptr(ws), nbytes, _stream_ptr(dev))
    return {"labels": labels, "clean_mask": clean.view(torch.bool), "table": table, "counts": counts}


def instance_records(table, counts, H, W):
    """The per-instance ratios of include/camo_instances.h from ``mask_instances``' table and counts (tensors or nested lists; a
    device tensor costs the one host copy), in float64 from the exact integers.  Per image a dict {"instances": [{"id", "area",
    "box": (x0, y0, x1, y1) inclusive, "centroid": (Sx / area, Sy / area), "score": Sq / (255 area)} in id order], "count": K,
    "truncated": K > the rows the table holds, "dropped", "holes", "pixels", "coverage": pixels / (H W)}."""
    if isinstance(table, torch.Tensor) and isinstance(counts, torch.Tensor) and table.is_cuda:
        flat = torch.cat([table.reshape(-1), counts.to(device=table.device, dtype=torch.int64).reshape(-1)]).tolist()      # (the one copy)
        nt = table.numel()
        rows_per = table.shape[1]
        cnt = [flat[nt + _lib.INST_COUNTS * i: nt + _lib.INST_COUNTS * (i + 1)] for i in range(counts.shape[0])]
        tab = [[flat[(i * rows_per + k) * _lib.INST_FIELDS: (i * rows_per + k + 1) * _lib.INST_FIELDS] for k in range(rows_per)]
               for i in range(table.shape[0])]
    else:
        tab = table.tolist() if isinstance(table, torch.Tensor) else [[list(r) for r in img] for img in table]
        cnt = counts.tolist() if isinstance(counts, torch.Tensor) else [list(c) for c in counts]
    if len(tab) != len(cnt):
        raise ValueError(f"table holds {len(tab)} images, counts {len(cnt)}")
    hw = float(H) * float(W)
    out = []
    for rows, c in zip(tab, cnt):
        if len(c) != _lib.INST_COUNTS or any(len(r) != _lib.INST_FIELDS for r in rows):
            raise ValueError(f"need table rows of {_lib.INST_FIELDS} and counts rows of {_lib.INST_COUNTS} integers")
        K, dropped, holes, pixels = (int(v) for v in c)
        inst = []
        for k in range(min(K, len(rows))):
            area, x0, y0, x1, y1, sx, sy, sq = (int(v) for v in rows[k])
            inst.append({"id": k + 1, "area": area, "box": (x0, y0, x1, y1), "centroid": (sx / area, sy / area), "score": sq / (255 * area)})
        out.append({"instances": inst, "count": K, "truncated": K > len(rows), "dropped": dropped, "holes": holes, "pixels": pixels,
                    "coverage": pixels / hw})
    return out


@torch.no_grad()
def detect_instances(pred, threshold=0.5, connectivity=8, min_area=0, fill_holes=False, max_instances=64):
    """``mask_instances`` and ``instance_records`` together: ``mask_instances``' dict plus "instances" (``instance_records``' list).
    When an image holds more than ``max_instances`` instances the call is made once more with the table sized to the largest count,
    so no list is truncated."""
    out = mask_instances(pred, threshold, connectivity, min_area, fill_holes, max_instances)
    H, W = out["labels"].shape[1:]
    rec = instance_records(out["table"], out["counts"], H, W)
    if any(r["truncated"] for r in rec):
        out = mask_instances(pred, threshold, connectivity, min_area, fill_holes, max(r["count"] for r in rec))
        rec = instance_records(out["table"], out["counts"], H, W)
    out["instances"] = rec
    return out
