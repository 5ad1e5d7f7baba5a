"""Instance contours on MI355X (include/camo_contours.h): label maps out as COCO polygons.

``trace_contours`` runs ``camo_contours`` on the label maps ``mask_instances`` writes -- the closed rings of every id, their vertices
on the integer corners of the pixels -- and returns device tensors; ``polygons_from_contours`` groups the rings by id on the host
into COCO polygon lists; ``encode_instance_polygons`` is the two together with a capacity that always holds every crack;
``coco_annotations`` writes them as the ``images`` and ``annotations`` of a COCO dataset, the form ``polygons.coco_ground_truth``
reads.  A polygon list is a union, so a reader (``polygons.decode_polygons``, pycocotools) rebuilds an instance with its holes
filled: exact for instances without holes (``fill_holes=True``), and "holes" carries the rings to subtract otherwise.
PARITY UNPINNED: the header's text is the definition (restated sequentially in numpy in tests/contours_ref.py).  Out of scope:
simplifying an outline, ``iscrowd``.  There is no CPU path for the label maps: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, label_map, workspace


def _check_connectivity(connectivity):
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _capacity(value, name, default, n_images, limit, limit_name):
    if value is None:
        value = default
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {value!r}")
    if n_images * value > limit:
        raise ValueError(f"{name} = {value} for {n_images} images exceeds {limit_name} = {limit}")
    return int(value)


@torch.no_grad()
def trace_contours(labels, connectivity=8, max_cracks=None, max_rings=None, max_vertices=None):
    """``camo_contours``: ``labels`` int32 [N, H, W] (or [H, W]) -> {"rings": int64 [N, max_rings, 5] = (label, first crack, offset of
    the first vertex in the image's xy, vertex count, a2) of every ring in order of first crack, "xy": int32 [N, max_vertices, 2], the
    rings' vertices (x, y) back to back, "counts": int32 [N, 6] = (cracks, rings, vertices the image holds; cracks taken, rings and
    vertices written)}, on the device, no host synchronisation.  ``max_cracks`` defaults to min(4 H W, CONTOUR_LDS_CRACKS),
    ``max_vertices`` to ``max_cracks`` and ``max_rings`` to max(1, max_cracks // 4): a ring has at least four cracks and vertices
    never outnumber cracks, so with the defaults only the crack capacity can overflow -- an image with more cracks takes none and
    its first count says what to ask for."""
    labels = label_map(labels, "labels")
    N, H, W = labels.shape
    connectivity = _check_connectivity(connectivity)
    C = _capacity(max_cracks, "max_cracks", min(4 * H * W, _lib.CONTOUR_LDS_CRACKS), N, _lib.CONTOUR_MAX_CRACKS, "CONTOUR_MAX_CRACKS")
    if C > 4 * H * W:
        raise ValueError(f"max_cracks = {C} exceeds 4 H W = {4 * H * W}: a pixel has four sides")
    R = _capacity(max_rings, "max_rings", max(1, C // 4), N, _lib.CONTOUR_MAX_RINGS, "CONTOUR_MAX_RINGS")
    V = _capacity(max_vertices, "max_vertices", C, N, _lib.CONTOUR_MAX_VERTICES, "CONTOUR_MAX_VERTICES")
    _lib.require_device(labels, "labels")
    labels = labels.detach().contiguous()
    dev = labels.device
    ws, nbytes = workspace("camo_contours_workspace_bytes", N, H, W, C, R, V, device=dev,
                           refuse=lambda: ValueError(f"camo_contours does not support N = {N}, H = {H}, W = {W}, max_cracks = {C}, max_rings = {R}, max_vertices = {V}"))
    rings = torch.empty(N, R, _lib.CONTOUR_RING_FIELDS, dtype=torch.int64, device=dev)
    xy = torch.empty(N, V, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(N, _lib.CONTOUR_COUNTS, dtype=torch.int32, device=dev)
    call("camo_contours", dev, _ptr(labels), N, H, W, connectivity, C, R, V, _ptr(rings), _ptr(xy), _ptr(counts), _ptr(ws), nbytes, _stream_ptr(dev))
    return {"rings": rings, "xy": xy, "counts": counts}


def _host_contours(rings, xy, counts):
    """(rings [N, R, 5], xy [N, V, 2], counts [N, 6]) as numpy arrays; three device tensors cost the ONE host copy."""
    if all(isinstance(t, torch.Tensor) for t in (rings, xy, counts)) and rings.is_cuda:
        parts = [t.to(rings.device).contiguous().reshape(-1).view(torch.uint8) for t in (rings, xy, counts)]      # (rings first: 8-byte aligned)
        flat = torch.cat(parts).cpu().numpy()                        # (the one copy)
        a, b = parts[0].numel(), parts[0].numel() + parts[1].numel()
        return (flat[:a].view(np.int64).reshape(tuple(rings.shape)), flat[a:b].view(np.int32).reshape(tuple(xy.shape)),
                flat[b:].view(np.int32).reshape(tuple(counts.shape)))
    return tuple(t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (rings, xy, counts))


def polygons_from_contours(rings, xy, counts):
    """Per image {id: {"polygons": [[x0, y0, x1, y1, ...], ...], "holes": [[...], ...], "area": int}} in id order, from
    ``trace_contours``' tensors (or arrays of their shapes): "polygons" are the id's outer rings (a2 > 0) in ring order, "holes" its
    rings with a2 < 0, "area" half the sum of its a2, which is its pixel count.  A polygon list is a union: painting "polygons"
    back gives the id with its holes filled, and "holes" is what to subtract.  An image whose cracks were not taken, or whose rings
    or vertices were not all written, raises ``ValueError`` naming the image and the capacity to ask for."""
    r, v, c = _host_contours(rings, xy, counts)
    if r.ndim == 2:
        r, v, c = r[None], v[None], np.reshape(c, (1, -1))
    if r.ndim != 3 or r.shape[2] != _lib.CONTOUR_RING_FIELDS or v.ndim != 3 or v.shape[2] != 2 or v.shape[0] != r.shape[0] or \
            c.shape != (r.shape[0], _lib.CONTOUR_COUNTS):
        raise ValueError(f"need rings [N, R, 5], xy [N, V, 2] and counts [N, 6], got {r.shape}, {v.shape} and {c.shape}")
    out = []
    for n in range(r.shape[0]):
        E, M, T, taken, rows, wrote = (int(x) for x in c[n])
        if E > taken:
            raise ValueError(f"image {n} holds {E} cracks and {taken} were taken: call trace_contours with max_cracks >= {E}")
        if M > rows:
            raise ValueError(f"image {n} holds {M} rings and {rows} were written: call trace_contours with max_rings >= {M}")
        if T > wrote:
            raise ValueError(f"image {n} holds {T} vertices and {wrote} were written: call trace_contours with max_vertices >= {T}")
        per_id = {}
        for label, _, off, nv, a2 in r[n, :M].tolist():
            entry = per_id.setdefault(label, {"polygons": [], "holes": [], "area": 0})
            entry["polygons" if a2 > 0 else "holes"].append(v[n, off:off + nv].reshape(-1).tolist())
            entry["area"] += a2
        for entry in per_id.values():
            entry["area"] //= 2
        out.append({k: per_id[k] for k in sorted(per_id)})
    return out


@torch.no_grad()
def encode_instance_polygons(labels, connectivity=8):
    """``trace_contours`` and ``polygons_from_contours`` together: per image {id: {"polygons", "holes", "area"}} of ``labels`` int32
    [N, H, W] (or [H, W]).  When an image holds more cracks than the default capacity the call is made once more with the capacity
    of the largest count, so no outline is cut short.  Host copies: the counts (once more after a second call), then the rows that hold
    a ring or a vertex.
    ``polygons.decode_polygons`` of the "polygons", each with its id as value, gives the label map back when no instance has a hole."""
    labels = label_map(labels, "labels")
    out = trace_contours(labels, connectivity)
    c = out["counts"].cpu().numpy()
    if (c[:, 0] > c[:, 3]).any():
        out = trace_contours(labels, connectivity, max_cracks=int(c[:, 0].max()))
        c = out["counts"].cpu().numpy()
    rows, verts = max(int(c[:, 4].max()), 1), max(int(c[:, 5].max()), 1)
    return polygons_from_contours(out["rings"][:, :rows], out["xy"][:, :verts], c)


def contour_options(polygons, instances=True):
    """The pipeline's ``polygons`` keyword as a bool; the ``ValueError`` of a bad one by name."""
    if not isinstance(polygons, bool):
        raise ValueError(f"polygons must be True or False, got {polygons!r}")
    if polygons and not instances:
        raise ValueError("polygons needs instances=True: the instances are what it outlines")
    return polygons


def coco_annotations(stems, sizes, instances, polygons, image_ids=None, category_id=1):
    """The ``images`` and ``annotations`` lists of a COCO dataset for some images: ``sizes`` per image (height, width), ``instances``
    per image the records of ``instance_records``, ``polygons`` per image ``encode_instance_polygons``' {id: ...}.  An image is
    {"id": the stem or ``image_ids[stem]``, "file_name": the stem, "height", "width"}; an instance {"id": 1, 2, ... over the call,
    "image_id", "category_id", "segmentation": its outer rings, "holes": its hole rings (no COCO field: a reader that paints
    "segmentation" gets the instance with its holes filled), "area": its pixel count, "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1],
    "iscrowd": 0, "score": the record's Sq / (255 area)}."""
    images, annotations = [], []
    for stem, (h, w), rec, enc in zip(stems, sizes, instances, polygons):
        image_id = stem if image_ids is None else image_ids[stem]
        images.append({"id": image_id, "file_name": stem, "height": int(h), "width": int(w)})
        for inst in rec["instances"]:
            x0, y0, x1, y1 = inst["box"]
            traced = enc[inst["id"]]
            annotations.append({"id": len(annotations) + 1, "image_id": image_id, "category_id": category_id, "segmentation": traced["polygons"],
                                "holes": traced["holes"], "area": traced["area"], "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1], "iscrowd": 0,
                                "score": inst["score"]})
    return images, annotations
