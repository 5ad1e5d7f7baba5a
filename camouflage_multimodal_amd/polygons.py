"""COCO polygon annotations on MI355X (include/camo_poly.h): a ``segmentation`` field in, an int32 label map out.

``decode_polygon_arrays`` is ``camo_poly_decode`` on host arrays; ``decode_polygons`` takes per image a list of COCO polygon lists
(``[[x0, y0, x1, y1, ...], ...]``) and paints them on the device; ``polygons_to_rles`` is COCO's frPyObjects + merge (one RLE per
annotation); ``decode_segmentations`` takes ``segmentation`` fields verbatim, polygons and RLEs mixed; ``coco_ground_truth`` reads
them off a COCO annotations file for a list of file names.
PARITY UNPINNED: the header's text is the definition (restated sequentially in numpy in tests/poly_ref.py).  Out of scope:
``iscrowd`` (crowd annotations are left out and counted), IoU in the RLE domain.  There is no CPU path for the label maps.
"""
from __future__ import annotations

import json
import numbers
import os

import numpy as np
import torch

from . import _lib, rle as _rle
from ._lib import _ptr, _stream_ptr, call, workspace

MAX_BOUNDARY_POINTS = 1 << 28        # the sum of n_j the header's PRECONDITION allows


def _no_cpu(dev):
    return _lib.CamoError(f"the label maps are painted on {dev}: camo_poly_decode runs as HIP kernels on an MI355X and has no CPU fallback")


def _size(H, W):
    for v, name in ((H, "H"), (W, "W")):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(H), int(W)


def boundary_points(xy, poly_off):
    """The sum of n_j of include/camo_poly.h, step 2, over every polygon (vectorised; coordinates that are not finite count as 0)."""
    xy = np.nan_to_num(np.asarray(xy, np.float64).reshape(-1, 2), nan=0.0, posinf=0.0, neginf=0.0)
    if xy.shape[0] == 0:
        return 0
    q = np.trunc(5.0 * np.clip(xy, -2.0 ** 40, 2.0 ** 40) + 0.5).astype(np.int64)
    nxt = np.arange(1, xy.shape[0] + 1)
    off = np.asarray(poly_off, np.int64)
    last = off[1:][off[1:] > off[:-1]] - 1                            # a polygon's last vertex is followed by its first
    nxt[last] = off[:-1][off[1:] > off[:-1]]
    return int((np.abs(q[nxt] - q).max(axis=1) + 1).sum())


@torch.no_grad()
def decode_polygon_arrays(xy, poly_off, ann_poly_off, ann_image, ann_value, N, H, W, device="cuda"):
    """``camo_poly_decode`` on host arrays: ``xy`` float64 [V, 2], the vertices of P polygons back to back, ``poly_off`` int32
    [P + 1] non-decreasing from 0 to V, ``ann_poly_off`` int32 [A + 1] non-decreasing from 0 to P, ``ann_image`` [A] and
    ``ann_value`` [A] -> (labels int32 [N, H, W], ann_area int64 [A]) on ``device``, no host synchronisation after the upload.  The
    arrays go up in ONE copy.  ``ann_area`` is the pixel count of an annotation's union, -1 for one that paints nothing: an image
    outside the batch, a value below 1, a polygon without a vertex or with a coordinate that is not finite or lies more than
    CAMO_POLY_MARGIN outside the image."""
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
    poly_off, ann_poly_off = np.asarray(poly_off, np.int32).reshape(-1), np.asarray(ann_poly_off, np.int32).reshape(-1)
    ann_image, ann_value = np.asarray(ann_image, np.int32).reshape(-1), np.asarray(ann_value, np.int32).reshape(-1)
    A, P, V = ann_image.size, poly_off.size - 1, xy.shape[0]
    H, W = _size(H, W)
    if isinstance(N, bool) or not isinstance(N, numbers.Integral) or N < 1:
        raise ValueError(f"N must be an integer >= 1, got {N!r}")
    if not 1 <= A <= _lib.POLY_MAX_ANNOTATIONS:
        raise ValueError(f"need 1 .. {_lib.POLY_MAX_ANNOTATIONS} annotations, got {A}")
    if ann_value.size != A or ann_poly_off.size != A + 1 or P < 0:
        raise ValueError(f"need ann_poly_off of {A + 1}, ann_value of {A} and poly_off of at least 1 integers, got {ann_poly_off.size}, {ann_value.size} and {poly_off.size}")
    if P > _lib.POLY_MAX_POLYGONS:
        raise ValueError(f"{P} polygons exceed {_lib.POLY_MAX_POLYGONS}")
    if V > _lib.POLY_MAX_VERTICES:
        raise ValueError(f"{V} vertices exceed {_lib.POLY_MAX_VERTICES}")
    if poly_off[0] != 0 or poly_off[-1] != V or (np.diff(poly_off) < 0).any():
        raise ValueError(f"poly_off must be non-decreasing from 0 to the number of vertices, {V}")
    if ann_poly_off[0] != 0 or ann_poly_off[-1] != P or (np.diff(ann_poly_off) < 0).any():
        raise ValueError(f"ann_poly_off must be non-decreasing from 0 to the number of polygons, {P}")
    if P * ((H * W + 31) // 32) > _lib.POLY_MAX_PLANE_WORDS:
        raise ValueError(f"{P} polygons on {H} x {W} need more than {_lib.POLY_MAX_PLANE_WORDS} plane words")
    points = boundary_points(xy, poly_off)
    if points > MAX_BOUNDARY_POINTS:
        raise ValueError(f"the polygons have {points} boundary points, more than {MAX_BOUNDARY_POINTS}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _no_cpu(dev)
    ws, nbytes = workspace("camo_poly_decode_workspace_bytes", int(N), H, W, A, P, V, device=dev,
                           refuse=lambda: ValueError(f"camo_poly_decode does not support N = {N}, H = {H}, W = {W}, {A} annotations, {P} polygons, {V} vertices"))
    ints = np.concatenate([poly_off, ann_poly_off, ann_image, ann_value])
    up = torch.from_numpy(np.concatenate([xy.reshape(-1).view(np.uint8), ints.view(np.uint8)])).to(dev)      # (the one copy; xy first: 8-byte aligned)
    at = [16 * V + 4 * v for v in (0, P + 1, P + A + 2, P + 2 * A + 2)]
    d_xy, d_poff, d_aoff, d_img, d_val = up[:16 * V], up[at[0]:at[1]], up[at[1]:at[2]], up[at[2]:at[3]], up[at[3]:]
    labels = torch.empty(int(N), H, W, dtype=torch.int32, device=dev)
    area = torch.empty(A, dtype=torch.int64, device=dev)
    call("camo_poly_decode", dev, _ptr(d_xy) if V else None, V, _ptr(d_poff), P, _ptr(d_aoff), _ptr(d_img), _ptr(d_val), A, int(N), H, W,
         _ptr(labels), _ptr(area), _ptr(ws), nbytes, _stream_ptr(dev))
    return labels, area


def _is_pair(ann, first):
    return isinstance(ann, (list, tuple)) and len(ann) == 2 and isinstance(ann[0], first) and isinstance(ann[1], (numbers.Integral, bool))


def _value(value, what):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not 1 <= value <= 2 ** 31 - 1:
        raise ValueError(f"{what}: the value must be an integer in [1, 2^31 - 1], got {value!r}")
    return int(value)


def _polygon_list(polygons, H, W, scale, what):
    """The [k, 2] float64 arrays of one annotation's polygon list, scaled and checked."""
    if not isinstance(polygons, (list, tuple)):
        raise ValueError(f"{what}: need a list of polygons [[x0, y0, x1, y1, ...], ...], got {type(polygons).__name__}")
    out = []
    for poly in polygons:
        try:
            c = np.asarray(poly, np.float64)
        except (TypeError, ValueError):
            c = None
        if c is None or c.ndim != 1 or isinstance(poly, (str, bytes)):
            raise ValueError(f"{what}: a polygon must be a flat list of numbers [x0, y0, x1, y1, ...], got {poly!r}")
        if c.size == 0:
            raise ValueError(f"{what}: an empty polygon")
        if c.size % 2:
            raise ValueError(f"{what}: a polygon with an odd number of coordinates, {c.size}")
        c = c.reshape(-1, 2)
        if scale is not None:
            c = c * scale                                             # (float64, on the host)
        if not np.isfinite(c).all():
            raise ValueError(f"{what}: a coordinate is not finite")
        m = _lib.POLY_MARGIN
        if (c < -m).any() or (c[:, 0] > W + m).any() or (c[:, 1] > H + m).any():
            raise ValueError(f"{what}: a coordinate lies more than {m} pixels outside the {H} x {W} image")
        out.append(c)
    return out


def _flatten(per_image, H, W, image_numbers, scales, numbered=False):
    """``decode_polygons``' argument as per-annotation (image, value, [k, 2] arrays); every ``ValueError`` by image and annotation.
    ``numbered``: the annotations come as (number, polygons, value) from ``decode_segmentations``."""
    if not isinstance(per_image, (list, tuple)) or not per_image:
        raise ValueError("per_image_annotations must be a non-empty list with one list of annotations per image")
    if image_numbers is not None and len(image_numbers) != len(per_image):
        raise ValueError(f"{len(image_numbers)} image numbers for {len(per_image)} images")
    if scales is not None and len(scales) != len(per_image):
        raise ValueError(f"{len(scales)} scales for {len(per_image)} images")
    anns_out = []
    for i, anns in enumerate(per_image):
        n = i if image_numbers is None else image_numbers[i]
        if not isinstance(anns, (list, tuple)):
            raise ValueError(f"image {n}: need a list of polygon lists or (polygons, value) pairs, got {type(anns).__name__}")
        scale = None
        if scales is not None:
            try:
                scale = np.asarray([float(scales[i][0]), float(scales[i][1])], np.float64)
            except (TypeError, ValueError, IndexError):
                scale = None
            if scale is None or len(scales[i]) != 2 or not np.isfinite(scale).all() or (scale <= 0).any():
                raise ValueError(f"image {n}: the scale must be two positive numbers (sx, sy), got {scales[i]!r}")
        for k, ann in enumerate(anns):
            if numbered:
                k, polygons, value = ann
            else:
                polygons, value = (ann[0], ann[1]) if _is_pair(ann, (list, tuple)) else (ann, k + 1)
            what = f"image {n}, annotation {k}"
            anns_out.append((i, _value(value, what), _polygon_list(polygons, H, W, scale, what), what))
    return anns_out


def _arrays(anns):
    xy = [c for _, _, polys, _ in anns for c in polys]
    poly_off = np.concatenate([[0], np.cumsum([len(c) for c in xy])]).astype(np.int64)
    ann_poly_off = np.concatenate([[0], np.cumsum([len(polys) for _, _, polys, _ in anns])]).astype(np.int64)
    flat = np.concatenate(xy) if xy else np.zeros((0, 2), np.float64)
    return flat, poly_off, ann_poly_off, np.asarray([a[0] for a in anns], np.int32), np.asarray([a[1] for a in anns], np.int32)


def _decode_flat(anns, N, H, W, dev):
    """(labels, areas) of ``_flatten``'s annotations; the call is split over annotations while its planes exceed the limit."""
    if len(anns) > _lib.POLY_MAX_ANNOTATIONS:
        raise ValueError(f"{len(anns)} annotations exceed {_lib.POLY_MAX_ANNOTATIONS}")
    n_poly, n_vert = sum(len(a[2]) for a in anns), sum(len(c) for a in anns for c in a[2])
    if n_poly > _lib.POLY_MAX_POLYGONS:
        raise ValueError(f"{n_poly} polygons exceed {_lib.POLY_MAX_POLYGONS}")
    if n_vert > _lib.POLY_MAX_VERTICES:
        raise ValueError(f"{n_vert} vertices exceed {_lib.POLY_MAX_VERTICES}")
    words = (H * W + 31) // 32
    room = _lib.POLY_MAX_PLANE_WORDS // words                         # polygons a call may hold
    parts, held = [[]], 0
    for a in anns:
        if len(a[2]) > room:
            raise ValueError(f"{a[3]}: {len(a[2])} polygons on {H} x {W} need more than {_lib.POLY_MAX_PLANE_WORDS} plane words")
        if held + len(a[2]) > room and parts[-1]:
            parts.append([])
            held = 0
        parts[-1].append(a)
        held += len(a[2])
    flats = [_arrays(p) for p in parts]
    points = sum(boundary_points(f[0], f[1]) for f in flats)
    if points > MAX_BOUNDARY_POINTS:
        raise ValueError(f"the polygons have {points} boundary points, more than {MAX_BOUNDARY_POINTS}")
    if dev.type != "cuda":
        raise _no_cpu(dev)
    labels, areas = None, []
    for f in flats:
        lab, area = decode_polygon_arrays(*f, N, H, W, dev)
        labels = lab if labels is None else torch.maximum(labels, lab)
        areas.append(area)
    return labels, areas[0] if len(areas) == 1 else torch.cat(areas)


@torch.no_grad()
def decode_polygons(per_image_annotations, H, W, device="cuda", image_numbers=None, scales=None, return_area=False):
    """``camo_poly_decode``: ``per_image_annotations`` -- per image a list of annotations, each a COCO polygon list
    ``[[x0, y0, x1, y1, ...], ...]`` or a (polygons, value) pair -- painted into ``labels`` int32 [N, H, W] on ``device``.  Values
    default to 1 .. K in list order; where annotations overlap the largest value wins.  ``scales[i] = (sx, sy)`` multiplies image i's
    coordinates (float64, on the host): ground truth given in native coordinates, painted at a working size.  An annotation with an
    empty polygon list is valid and paints nothing; a polygon with no or an odd number of coordinates, a coordinate that is not finite
    or lies more than CAMO_POLY_MARGIN outside the image, a bad value and too many annotations, polygons, vertices or boundary points
    raise ``ValueError`` naming the image and the annotation, on the host before anything is uploaded (``image_numbers``: the numbers
    the messages give the images).  When the polygons' bit-planes exceed CAMO_POLY_MAX_PLANE_WORDS the call is split over annotations
    and the maps are combined by maximum.  ``return_area=True``: (labels, int64 [annotations] pixel counts in list order)."""
    H, W = _size(H, W)
    anns = _flatten(per_image_annotations, H, W, image_numbers, scales)
    dev = torch.device(device)
    N = len(per_image_annotations)
    if not anns:                                                     # no annotation at all: nothing to paint
        if dev.type != "cuda":
            raise _no_cpu(dev)
        labels, area = torch.zeros(N, H, W, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev)
    else:
        labels, area = _decode_flat(anns, N, H, W, dev)
    return (labels, area) if return_area else labels


@torch.no_grad()
def polygons_to_rles(annotations, H, W, device="cuda"):
    """COCO's frPyObjects + merge for one image size: ``annotations`` is a list of polygon lists, the result one
    {"size": [H, W], "counts": str} per annotation (the union of its polygons).  Every annotation is painted into an image slot of
    its own, so overlapping annotations keep their own pixels; a call's label maps stay under 2^26 pixels.  A ``ValueError`` names
    the annotation by its place in the list."""
    H, W = _size(H, W)
    if not isinstance(annotations, (list, tuple)):
        raise ValueError(f"annotations must be a list of polygon lists, got {type(annotations).__name__}")
    chunk = max(1, min(((1 << 26) - 1) // (H * W), 65535))
    flat = [(k % chunk, 1, _polygon_list(a, H, W, None, f"annotation {k}"), f"annotation {k}") for k, a in enumerate(annotations)]
    checked = [flat[at:at + chunk] for at in range(0, len(flat), chunk)]      # (every annotation is checked before any is painted)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _no_cpu(dev)
    empty = {"size": [H, W], "counts": _rle.counts_to_string([H * W])}
    out = []
    for anns in checked:
        labels, _ = _decode_flat(anns, len(anns), H, W, dev)
        out += [enc.get(1, dict(empty)) for enc in _rle.encode_instances(labels)]
    return out


@torch.no_grad()
def decode_segmentations(per_image, H, W, device="cuda", image_numbers=None):
    """COCO ``segmentation`` fields verbatim -> ``labels`` int32 [N, H, W] on ``device``: per image a list whose entries are a polygon
    list, an RLE dict ({"size", "counts"}: a string or a list) or a (segmentation, value) pair.  Values default to 1 .. K in list order
    across both kinds.  Polygons go through ``decode_polygons``, RLEs through ``rle.decode_rles``, and the maps are combined by
    maximum.  Every ``ValueError`` names the image and the annotation, before anything is uploaded."""
    H, W = _size(H, W)
    if not isinstance(per_image, (list, tuple)) or not per_image:
        raise ValueError("per_image must be a non-empty list with one list of segmentations per image")
    if image_numbers is not None and len(image_numbers) != len(per_image):
        raise ValueError(f"{len(image_numbers)} image numbers for {len(per_image)} images")
    polys, rles = [], []
    for i, anns in enumerate(per_image):
        n = i if image_numbers is None else image_numbers[i]
        if not isinstance(anns, (list, tuple)):
            raise ValueError(f"image {n}: need a list of segmentations or (segmentation, value) pairs, got {type(anns).__name__}")
        polys.append([]); rles.append([])
        for k, ann in enumerate(anns):
            what = f"image {n}, annotation {k}"
            seg, value = (ann[0], ann[1]) if _is_pair(ann, (list, tuple, dict)) else (ann, k + 1)
            value = _value(value, what)
            if isinstance(seg, dict):
                cnts, _ = _rle._rle_counts(seg, H, W, what)
                if int(cnts.sum()) != H * W:
                    raise ValueError(f"{what}: the counts sum to {int(cnts.sum())}, the image has {H * W} pixels")
                rles[-1].append((seg, value))
            elif isinstance(seg, (list, tuple)):
                polys[-1].append((k, seg, value))
            else:
                raise ValueError(f"{what}: a segmentation is a polygon list or an RLE dict, got {type(seg).__name__}")
    flat = _flatten(polys, H, W, image_numbers, None, numbered=True)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _no_cpu(dev)
    N = len(per_image)
    labels = _decode_flat(flat, N, H, W, dev)[0] if flat else None
    if any(rles):
        painted = _rle.decode_rles(rles, H, W, dev, image_numbers)
        labels = painted if labels is None else torch.maximum(labels, painted)
    return labels if labels is not None else torch.zeros(N, H, W, dtype=torch.int32, device=dev)


def _stem(name):
    return os.path.splitext(os.path.basename(str(name)))[0]


def coco_ground_truth(annotations, names):
    """The ground truth of some images off a COCO annotations file: ``annotations`` is its path or the loaded dict, ``names`` file
    names or stems in the caller's order.  Returns {"segmentations": per name the ``segmentation`` fields of its annotations in file
    order (``decode_segmentations``' argument), "sizes": [(height, width)], "image_ids": {stem: id}, "crowd_skipped": n}.  Annotations
    with ``iscrowd`` = 1 are left out and counted.  A name the file does not hold, and a stem that more than one of its images has, raise ``ValueError`` and
    name it."""
    if isinstance(annotations, (str, os.PathLike)):
        with open(annotations) as f:
            annotations = json.load(f)
    if not isinstance(annotations, dict) or not isinstance(annotations.get("images"), list) or not isinstance(annotations.get("annotations"), list):
        raise ValueError('annotations must be a COCO annotations file (a path or its dict) with "images" and "annotations"')
    by_name, by_stem, shared = {}, {}, set()
    for im in annotations["images"]:
        by_name[im["file_name"]] = im
        if by_stem.setdefault(_stem(im["file_name"]), im) is not im:
            shared.add(_stem(im["file_name"]))                        # two files of one stem, in different folders
    per_id, crowd = {}, 0
    for ann in annotations["annotations"]:
        if ann.get("iscrowd", 0):
            crowd += 1
            continue
        per_id.setdefault(ann["image_id"], []).append(ann["segmentation"])
    segs, sizes, ids = [], [], {}
    for name in names:
        if name not in by_name and (name if name in by_stem else _stem(name)) in shared:
            raise ValueError(f"the annotations hold more than one image with the stem of {name!r}: give its file name as the annotations state it")
        im = by_name.get(name, by_stem.get(name, by_stem.get(_stem(name))))
        if im is None:
            raise ValueError(f"the annotations hold no image named {name!r}")
        segs.append(list(per_id.get(im["id"], [])))
        sizes.append((int(im["height"]), int(im["width"])))
        ids[name if name not in by_name and name in by_stem else _stem(name)] = im["id"]
    return {"segmentations": segs, "sizes": sizes, "image_ids": ids, "crowd_skipped": crowd}
