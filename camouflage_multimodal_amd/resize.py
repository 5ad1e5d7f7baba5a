"""Resize on the device: mixed-size images in, native-size masks out (include/camo_resize.h).

The data of this project are 8-bit files, each of its own size; the detector works at one fixed size and the benchmark tables are
scored at each ground truth's own size.  ``pack_images`` puts a list of uint8 images into one device buffer, ``resize_batch``
resamples them -- with a crop box and a flip per image -- to a fixed fp32 batch in ONE launch of ``camo_resize``, and
``resize_to_sizes`` takes fp32 maps back to ragged native sizes in one launch.  On top: ``detect_camouflage_ragged``,
``prepare_finetune_batch_ragged`` (``RegionGraphFineTuner.step_from_ragged`` / ``.evaluate_ragged``), ``random_resized_crops`` and
``detect_camouflage_directory``.  PARITY UNPINNED: cv2 and skimage are absent, so the header's text defines the filters (exact
integer arithmetic; tests/resize_ref.py restates it).  There is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import _lib, instance_match as _match, instances as _instances, polygons as _polygons, refine as _refine, rle as _rle, seg_measures
from .engine import _ptr, _stream_ptr
from .rg_detect import detect_camouflage_batch, segmentation_counts, segmentation_metrics
from .rg_finetune import prepare_finetune_batch

FILTERS = {"nearest": _lib.RSZ_NEAREST, "bilinear": _lib.RSZ_BILINEAR, "area": _lib.RSZ_AREA}
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp")


class RaggedImages:
    """uint8 images of mixed sizes in ONE device buffer: ``data`` uint8 [sum H_i W_i C] (image i packed HWC, one after the other),
    ``sizes`` the host list of (H_i, W_i), ``channels`` C; ``squeeze`` says the images came as [H, W] (C = 1)."""

    def __init__(self, data, sizes, channels, squeeze=False):
        self.data, self.sizes, self.channels, self.squeeze = data, [(int(h), int(w)) for h, w in sizes], int(channels), bool(squeeze)

    def __len__(self):
        return len(self.sizes)

    def offsets(self):
        out, at = [], 0
        for h, w in self.sizes:
            out.append(at)
            at += h * w * self.channels
        return out

    def image(self, i):
        """Image i as a view [H, W, C] (or [H, W]) of ``data``."""
        h, w = self.sizes[i]
        o = self.offsets()[i]
        v = self.data[o:o + h * w * self.channels]
        return v.view(h, w) if self.squeeze else v.view(h, w, self.channels)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.CamoError(f"device {dev}: the resize runs as a HIP kernel on an MI355X and has no CPU fallback")
    if not torch.cuda.is_available():
        raise _lib.CamoError("no HIP device is available: the resize runs as a HIP kernel on an MI355X and has no CPU fallback")
    return dev


def pack_images(images, device="cuda"):
    """A list of uint8 [H_i, W_i] / [H_i, W_i, C] arrays or tensors (the same C throughout, bool is taken as 0 / 255) ->
    ``RaggedImages`` on ``device``.  Host inputs go through one pinned staging buffer and ONE host-to-device copy; inputs that are
    all on a device already go through one ``torch.cat``."""
    images = list(images)
    if not images:
        raise ValueError("pack_images needs at least one image")
    ts = []
    for k, im in enumerate(images):
        t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        if t.dtype == torch.bool:
            t = t.to(torch.uint8) * 255
        if t.dtype != torch.uint8 or t.dim() not in (2, 3) or t.numel() == 0:
            raise ValueError(f"image {k}: need uint8 [H, W] or [H, W, C], got {t.dtype} {tuple(t.shape)}")
        ts.append(t)
    squeeze = ts[0].dim() == 2
    C = 1 if squeeze else int(ts[0].shape[2])
    if any((t.dim() == 2) != squeeze or (not squeeze and t.shape[2] != C) for t in ts):
        raise ValueError("every image of a batch must have the same number of channels")
    if not 1 <= C <= _lib.RSZ_MAX_CHANNELS:
        raise ValueError(f"1 to {_lib.RSZ_MAX_CHANNELS} channels, got {C}")
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in ts]
    if all(t.is_cuda for t in ts):
        return RaggedImages(torch.cat([t.contiguous().reshape(-1) for t in ts]), sizes, C, squeeze)
    if any(t.is_cuda for t in ts):
        raise ValueError("the images of a batch must be all on the host or all on a device")
    dev = _device(device)
    stage = torch.empty(sum(t.numel() for t in ts), dtype=torch.uint8).pin_memory()
    at = 0
    for t in ts:
        stage[at:at + t.numel()].copy_(t.reshape(-1))
        at += t.numel()
    return RaggedImages(stage.to(dev, non_blocking=True), sizes, C, squeeze)


def check_table(rows, channels, src_elems, dst_elems, max_dst_pixels):
    """The row conditions of include/camo_resize.h on host integers: a bad row raises ``ValueError`` (the kernel would refuse it)."""
    S = _lib.RSZ_MAX_SIDE
    for i, r in enumerate(rows):
        if len(r) != _lib.RSZ_FIELDS:
            raise ValueError(f"row {i}: {len(r)} fields, need {_lib.RSZ_FIELDS}")
        so, sh, sw, srs, sps, scs, y0, x0, ch, cw, flip, do, dh, dw, drs, dps, dcs, rsv = (int(v) for v in r)
        if not all(1 <= v <= S for v in (sh, sw, ch, cw, dh, dw)):
            raise ValueError(f"image {i}: every side must be in [1, {S}]: source {sh} x {sw}, crop {ch} x {cw}, destination {dh} x {dw}")
        if y0 < 0 or x0 < 0 or y0 + ch > sh or x0 + cw > sw:
            raise ValueError(f"image {i}: the crop (y0, x0, h, w) = {(y0, x0, ch, cw)} does not lie inside the {sh} x {sw} image")
        if min(srs, sps, scs, drs, dps, dcs) < 1:
            raise ValueError(f"image {i}: strides must be >= 1")
        if not 0 <= flip <= 3:
            raise ValueError(f"image {i}: flip must be in 0..3, got {flip}")
        if rsv != 0 or so < 0 or do < 0:
            raise ValueError(f"image {i}: negative offset or non-zero reserved field")
        if so + (sh - 1) * srs + (sw - 1) * sps + (channels - 1) * scs >= src_elems:
            raise ValueError(f"image {i}: the source footprint leaves the source buffer")
        if do + (dh - 1) * drs + (dw - 1) * dps + (channels - 1) * dcs >= dst_elems:
            raise ValueError(f"image {i}: the destination footprint leaves the destination buffer")
        if dh * dw > max_dst_pixels:
            raise ValueError(f"image {i}: {dh} x {dw} destination pixels exceed max_dst_pixels = {max_dst_pixels}")


def _type_of(t, name):
    if t.dtype == torch.uint8:
        return _lib.RSZ_U8
    if t.dtype == torch.float32:
        return _lib.RSZ_F32
    raise ValueError(f"{name} must be uint8 or float32, got {t.dtype}")


@torch.no_grad()
def resize_table(src, dst, table, channels, filter="bilinear", max_dst_pixels=None, src_elems=None, dst_elems=None):
    """``camo_resize`` as it is: ``src`` / ``dst`` device tensors (uint8 or fp32) whose storage from ``data_ptr()`` on holds
    ``src_elems`` / ``dst_elems`` elements (default: ``numel()`` of a contiguous tensor), ``table`` int64 [N, 18] -- a device tensor
    is used unchecked (the kernel guards every row), anything else is checked with ``check_table`` and uploaded.  ``dst`` is
    written in place; returns the int32 [N] status tensor on the device (0 = row done, 1 = row refused and its destination
    zeroed), which nothing here reads back."""
    _lib.require_device(src, "src")
    _lib.require_device(dst, "dst")
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    dev = src.device
    if dst.device != dev:
        raise ValueError("src and dst must be on the same device")
    src_elems = int(src.numel() if src_elems is None else src_elems)
    dst_elems = int(dst.numel() if dst_elems is None else dst_elems)
    if isinstance(table, torch.Tensor) and table.is_cuda:
        tb = table.to(device=dev, dtype=torch.int64).contiguous()
        if max_dst_pixels is None:
            raise ValueError("a device table needs max_dst_pixels")
    else:
        rows = table.tolist() if isinstance(table, (torch.Tensor, np.ndarray)) else [list(r) for r in table]
        if max_dst_pixels is None:
            max_dst_pixels = max(int(r[12]) * int(r[13]) for r in rows)
        check_table(rows, channels, src_elems, dst_elems, int(max_dst_pixels))
        tb = torch.tensor(rows, dtype=torch.int64).to(dev)
    if tb.dim() != 2 or tb.shape[1] != _lib.RSZ_FIELDS or tb.shape[0] == 0:
        raise ValueError(f"need a table [N, {_lib.RSZ_FIELDS}], got {tuple(tb.shape)}")
    N = tb.shape[0]
    status = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().camo_resize(_ptr(src), src_elems, _type_of(src, "src"), _ptr(dst), dst_elems, _type_of(dst, "dst"), _ptr(tb), N,
                                    int(channels), FILTERS[filter], int(max_dst_pixels), _ptr(status), _stream_ptr(dev))
    _lib.check(rc, "camo_resize")
    return status


def _ragged(images, device="cuda"):
    """``images`` of ``resize_batch`` as (uint8 device buffer, per image (offset, H, W, row stride, pixel stride), C, squeeze)."""
    if isinstance(images, RaggedImages):
        _lib.require_device(images.data, "images")
        C = images.channels
        return images.data, [(o, h, w, w * C, C) for o, (h, w) in zip(images.offsets(), images.sizes)], C, images.squeeze
    if isinstance(images, torch.Tensor):
        _lib.require_device(images, "images")
        if images.dtype == torch.bool:
            images = images.to(torch.uint8) * 255
        if images.dtype != torch.uint8 or images.dim() not in (3, 4) or images.numel() == 0:
            raise ValueError(f"need uint8 images [N, H, W, C] or [N, H, W], got {images.dtype} {tuple(images.shape)}")
        t = images.contiguous()
        squeeze = t.dim() == 3
        N, H, W = t.shape[:3]
        C = 1 if squeeze else int(t.shape[3])
        return t, [(i * H * W * C, H, W, W * C, C) for i in range(N)], C, squeeze
    return _ragged(pack_images(images, device))


def _packed(data, geo, C):
    """A packed buffer with its geometry as the ``RaggedImages`` it is (the images of ``_ragged`` follow one another)."""
    return RaggedImages(data, [(g[1], g[2]) for g in geo], C)


def _boxes(crops, flips, geo):
    N = len(geo)
    if crops is None:
        crops = [(0, 0, g[1], g[2]) for g in geo]
    if flips is None:
        flips = [0] * N
    crops, flips = [tuple(int(v) for v in c) for c in crops], [int(f) for f in flips]
    if len(crops) != N or len(flips) != N or any(len(c) != 4 for c in crops):
        raise ValueError(f"need {N} crops (y0, x0, h, w) and {N} flips, got {len(crops)} and {len(flips)}")
    return crops, flips


@torch.no_grad()
def resize_batch(images, size=(256, 256), filter="bilinear", crops=None, flips=None, out_dtype=torch.float32):
    """``images`` -- a ``RaggedImages``, a list of uint8 images (packed first, see ``pack_images``) or a uint8 [N, H, W, C] /
    [N, H, W] device tensor -- resampled to ``size`` = (Ho, Wo) in ONE launch: fp32 [N, Ho, Wo, C] in [0, 1] (the exact filtered value
    over 255), or uint8 with ``out_dtype=torch.uint8`` (a half rounds up).  Images given as [H, W] come back [N, Ho, Wo].
    ``filter``: "nearest", "bilinear" (cv2.INTER_LINEAR's sampling) or "area" (cv2.INTER_AREA's box; bilinear on an axis that grows).
    ``crops``: N boxes (y0, x0, h, w) resampled in place of the whole images, the border repeated at the box's edge; ``flips``: N
    values, bit 0 mirrors columns and bit 1 rows.  A box outside its image, or any side above 8192, raises ``ValueError``."""
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
    Ho, Wo = (int(v) for v in size)
    data, geo, C, squeeze = _ragged(images)
    crops, flips = _boxes(crops, flips, geo)
    rows = [[o, h, w, rs, ps, 1, y0, x0, ch, cw, f, i * Ho * Wo * C, Ho, Wo, Wo * C, C, 1, 0]
            for i, ((o, h, w, rs, ps), (y0, x0, ch, cw), f) in enumerate(zip(geo, crops, flips))]
    if not (1 <= Ho <= _lib.RSZ_MAX_SIDE and 1 <= Wo <= _lib.RSZ_MAX_SIDE):
        raise ValueError(f"size must be within [1, {_lib.RSZ_MAX_SIDE}] a side, got {(Ho, Wo)}")
    out = torch.empty((len(geo), Ho, Wo) if squeeze else (len(geo), Ho, Wo, C), dtype=out_dtype, device=data.device)
    resize_table(data, out, rows, C, filter, Ho * Wo)
    return out


@torch.no_grad()
def resize_to_sizes(maps, sizes, filter="bilinear"):
    """fp32 ``maps`` [N, h, w] or [N, C, h, w] (a channel slice of a larger tensor is read in place through its strides) resampled
    to ``sizes``, N pairs (H_i, W_i), in ONE launch -> (list of N views [H_i, W_i] / [C, H_i, W_i], the ONE packed fp32 buffer they
    are views of).  ``filter``: "nearest" or "bilinear"."""
    _lib.require_device(maps, "maps")
    if maps.dtype != torch.float32 or maps.dim() not in (3, 4) or maps.numel() == 0:
        raise ValueError(f"need fp32 maps [N, h, w] or [N, C, h, w], got {maps.dtype} {tuple(maps.shape)}")
    if filter not in ("nearest", "bilinear"):
        raise ValueError(f'fp32 maps take filter "nearest" or "bilinear", got {filter!r}')
    maps = maps.detach()
    planar = maps.dim() == 4
    if any(s < 1 for s, n in zip(maps.stride(), maps.shape) if n > 1):
        maps = maps.contiguous()
    N, h, w = maps.shape[0], maps.shape[-2], maps.shape[-1]
    C = int(maps.shape[1]) if planar else 1
    st = [max(int(s), 1) for s in maps.stride()]            # (the stride of an axis of length 1 is never multiplied by anything but 0)
    s_img, s_ch, s_row, s_pix = (st[0], st[1], st[2], st[3]) if planar else (st[0], 1, st[1], st[2])
    sizes = [(int(a), int(b)) for a, b in sizes]
    if len(sizes) != N:
        raise ValueError(f"need {N} sizes, got {len(sizes)}")
    if any(a < 1 or b < 1 for a, b in sizes):
        raise ValueError("every size must be at least 1 x 1")
    src_elems = 1 + sum((n - 1) * s for n, s in zip(maps.shape, maps.stride()))
    rows, at = [], 0
    for i, (H, W) in enumerate(sizes):
        rows.append([i * s_img if N > 1 else 0, h, w, s_row, s_pix, s_ch, 0, 0, h, w, 0, at, H, W, W, 1, H * W, 0])
        at += C * H * W
    buf = torch.empty(at, dtype=torch.float32, device=maps.device)
    resize_table(maps, buf, rows, C, filter, max(H * W for H, W in sizes), src_elems=src_elems)
    views = []
    for r, (H, W) in zip(rows, sizes):
        v = buf[r[11]:r[11] + C * H * W]
        views.append(v.view(C, H, W) if planar else v.view(H, W))
    return views, buf


def random_resized_crops(sizes, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=0):
    """The boxes and flips of a RandomResizedCrop + RandomHorizontalFlip for images of ``sizes`` [(H, W), ...]: host only, driven by
    ``numpy.random.RandomState(seed)``, so the same seed gives the same list.  Per image up to ten draws of an area fraction in
    ``scale`` and an aspect ratio (w / h) log-uniform in ``ratio``; the first box that fits is placed uniformly inside the image;
    after ten rejected draws the box is the whole image.  Returns (crops [(y0, x0, h, w)], flips [0 or 1: mirror the columns])."""
    rs = np.random.RandomState(seed)
    crops, flips = [], []
    for H, W in sizes:
        H, W = int(H), int(W)
        box = (0, 0, H, W)
        for _ in range(10):
            area = H * W * rs.uniform(scale[0], scale[1])
            aspect = math.exp(rs.uniform(math.log(ratio[0]), math.log(ratio[1])))
            w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                box = (int(rs.randint(0, H - h + 1)), int(rs.randint(0, W - w + 1)), h, w)
                break
        crops.append(box)
        flips.append(1 if rs.uniform() < flip_p else 0)
    return crops, flips


def _mask_list(masks, n, name, device):
    """N masks (uint8 positive above 127, or bool) of mixed sizes as a ``RaggedImages`` of [H, W] bytes."""
    if isinstance(masks, RaggedImages):
        packed = masks
    elif isinstance(masks, torch.Tensor):
        if masks.dim() != 3:
            raise ValueError(f"need {name} [N, H, W] or a list of [H, W], got {tuple(masks.shape)}")
        packed = pack_images(list(masks), device)
    else:
        packed = pack_images(masks, device)
    if len(packed) != n or packed.channels != 1:
        raise ValueError(f"need {n} single-channel {name}, got {len(packed)} with {packed.channels} channels")
    return packed


def _score(preds, gts, threshold, cod, curves=False):
    """``segmentation_metrics`` (and ``seg_measures.cod_metrics``) of every fp32 [H_i, W_i] map against its uint8 mask of the same
    size; maps of equal size share a call.  Returns (metrics list, cod list or None) in the maps' order."""
    groups = {}
    for i, (p, g) in enumerate(zip(preds, gts)):
        if tuple(p.shape) != tuple(g.shape):
            raise ValueError(f"image {i}: the map is {tuple(p.shape)}, its mask {tuple(g.shape)}")
        groups.setdefault(tuple(p.shape), []).append(i)
    metrics, cods = [None] * len(preds), [None] * len(preds) if cod else None
    for (H, W), idx in groups.items():
        p, g = torch.stack([preds[i] for i in idx]), torch.stack([gts[i] for i in idx])
        for i, m in zip(idx, segmentation_metrics(segmentation_counts(p, g, threshold), H, W)):
            metrics[i] = m
        if cod:
            for i, m in zip(idx, seg_measures.cod_metrics(p, g, curves)):
                cods[i] = m
    return metrics, cods


def _native_instances(preds, threshold, connectivity, min_area, fill_holes):
    """``instances.detect_instances`` of every fp32 [H_i, W_i] map; maps of equal size share a call.  Returns (records, labels, clean
    masks, tables), four lists in the maps' order."""
    groups = {}
    for i, p in enumerate(preds):
        groups.setdefault(tuple(p.shape), []).append(i)
    rec, labels, clean, tables = [None] * len(preds), [None] * len(preds), [None] * len(preds), [None] * len(preds)
    for idx in groups.values():
        found = _instances.detect_instances(torch.stack([preds[i] for i in idx]), threshold, connectivity, min_area, fill_holes)
        for j, i in enumerate(idx):
            rec[i], labels[i], clean[i], tables[i] = found["instances"][j], found["labels"][j], found["clean_mask"][j], found["table"][j]
    return rec, labels, clean, tables


def _native_matches(labels, tables, gt_labels, opts):
    """``instance_match.match_detected`` of every int32 [H_i, W_i] label map against its ground-truth ids; maps of equal size share
    a call.  Returns (records, tables), two lists in the maps' order (a table dict holds the image's own rows)."""
    groups = {}
    for i, (p, g) in enumerate(zip(labels, gt_labels)):
        if tuple(p.shape) != tuple(g.shape):
            raise ValueError(f"image {i}: the label map is {tuple(p.shape)}, its ground truth {tuple(g.shape)}")
        groups.setdefault(tuple(p.shape), []).append(i)
    rec, out = [None] * len(labels), [None] * len(labels)
    for idx in groups.values():
        r, t = _match.match_detected(torch.stack([labels[i] for i in idx]), torch.stack([tables[i] for i in idx]),
                                     torch.stack([torch.as_tensor(gt_labels[i]).to(labels[i].device, torch.int32) for i in idx]), opts)
        for j, i in enumerate(idx):
            rec[i] = r[j]
            out[i] = {k: (v[j] if isinstance(v, torch.Tensor) else v) for k, v in t.items()}
    return rec, out


def _native_rles(labels):
    """``rle.encode_instances`` of every int32 [H_i, W_i] label map; maps of equal size share a call."""
    groups = {}
    for i, m in enumerate(labels):
        groups.setdefault(tuple(m.shape), []).append(i)
    out = [None] * len(labels)
    for idx in groups.values():
        enc = _rle.encode_instances(torch.stack([labels[i] for i in idx]))
        for j, i in enumerate(idx):
            out[i] = enc[j]
    return out


def _native_rle_labels(gt_rles, sizes, device):
    """``rle.decode_rles`` of every image's ground-truth RLEs at the image's own size; images of equal size share a call."""
    groups = {}
    for i, size in enumerate(sizes):
        groups.setdefault(tuple(size), []).append(i)
    out = [None] * len(sizes)
    for (H, W), idx in groups.items():
        lab = _rle.decode_rles([gt_rles[i] for i in idx], H, W, device, image_numbers=idx)
        for j, i in enumerate(idx):
            out[i] = lab[j]
    return out


def _native_segmentation_labels(gt_segmentations, sizes, device):
    """``polygons.decode_segmentations`` of every image's COCO segmentations at the image's own size; images of equal size share a call."""
    groups = {}
    for i, size in enumerate(sizes):
        groups.setdefault(tuple(size), []).append(i)
    out = [None] * len(sizes)
    for (H, W), idx in groups.items():
        lab = _polygons.decode_segmentations([gt_segmentations[i] for i in idx], H, W, device, image_numbers=idx)
        for j, i in enumerate(idx):
            out[i] = lab[j]
    return out


def _native_gt_labels(masks, connectivity, max_gt):
    """``instance_match.ground_truth_labels`` of every [H_i, W_i] mask; masks of equal size share a call."""
    groups = {}
    for i, m in enumerate(masks):
        groups.setdefault(tuple(m.shape), []).append(i)
    out = [None] * len(masks)
    for idx in groups.values():
        lab = _match.ground_truth_labels(torch.stack([masks[i] for i in idx]), connectivity, max_gt)
        for j, i in enumerate(idx):
            out[i] = lab[j]
    return out


@torch.no_grad()
def detect_camouflage_ragged(rg_model, images, gt_masks=None, size=(256, 256), n_segments=500, threshold=0.5, device="cuda",
                             cod_metrics=False, evaluate_at="native", instances=False, min_area=0, fill_holes=False, connectivity=8, refine=None,
                             *, match=None, rle=False):
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
    (``rle.encode_instances``; maps of equal size share a call)."""
    if instances:
        _instances.check_arguments(threshold, connectivity, min_area)
    rle = _rle.rle_options(rle, instances)
    match = _match.match_options(match, instances, gt_masks is not None and evaluate_at == "native")
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
    out = detect_camouflage_batch(rg_model, img, gt, n_segments, threshold, img.device, cod_metrics and resized, refine=refine)
    native, _ = resize_to_sizes(out["prob_maps"][:, 0], sizes, "bilinear")
    out["prob_maps_native"] = native
    out["mask_native"] = [p > threshold for p in native]
    if masks is not None and not resized:
        out["metrics"], cods = _score(native, [masks.image(i) for i in range(len(sizes))], threshold, cod_metrics)
        if cod_metrics:
            out["cod_metrics"] = cods
    if instances:
        rec, labels, clean, tables = _native_instances(native, threshold, connectivity, min_area, fill_holes)
        out.update({"instances_native": rec, "instance_labels_native": labels, "clean_mask_native": clean})
        if masks is not None and not resized:
            out["clean_metrics"], _ = _score([c.float() for c in clean], [masks.image(i) for i in range(len(sizes))], 0.5, False)
        if match is not None:
            gt_labels = match["gt_labels"]
            if match["gt_rles"] is not None:
                if len(match["gt_rles"]) != len(sizes):
                    raise ValueError(f'match["gt_rles"] holds {len(match["gt_rles"])} lists for {len(sizes)} images')
                gt_labels = _native_rle_labels(match["gt_rles"], sizes, img.device)
            elif match["gt_segmentations"] is not None:
                if len(match["gt_segmentations"]) != len(sizes):
                    raise ValueError(f'match["gt_segmentations"] holds {len(match["gt_segmentations"])} lists for {len(sizes)} images')
                gt_labels = _native_segmentation_labels(match["gt_segmentations"], sizes, img.device)
            elif gt_labels is None:
                gt_labels = _native_gt_labels([masks.image(i) for i in range(len(sizes))], connectivity, match["max_gt"])
            elif len(gt_labels) != len(sizes):
                raise ValueError(f'match["gt_labels"] holds {len(gt_labels)} maps for {len(sizes)} images')
            out["instance_match"], out["instance_match_tables"] = _native_matches(labels, tables, gt_labels, match)
        if rle:
            out["instance_rles_native"] = _native_rles(labels)
    if refine is not None:
        refined, _ = _refine.guided_upsample(out["refine_coefficients"], packed)
        out["prob_maps_native_refined"] = refined
        out["mask_native_refined"] = [p > threshold for p in refined]
        if masks is not None and not resized:
            out["refined_metrics"], cods = _score(refined, [masks.image(i) for i in range(len(sizes))], threshold, cod_metrics)
            if cod_metrics:
                out["refined_cod_metrics"] = cods
    return out


@torch.no_grad()
def prepare_finetune_batch_ragged(images, gt_masks, instance_masks=None, edge_masks=None, size=(256, 256), crops=None, flips=None, **kw):
    """``prepare_finetune_batch`` for uint8 images and masks of mixed sizes: the images are resized to ``size`` bilinear, every mask
    nearest, all with the same ``crops`` and ``flips`` (``random_resized_crops`` draws them), and the result goes to
    ``prepare_finetune_batch`` with ``**kw`` (n_segments, band_permille, device, edge_min_pixels)."""
    device = kw.get("device", "cuda")
    data, geo, C, _ = _ragged(images, device)
    if C != 3:
        raise ValueError(f"need images with 3 channels, got {C}")
    packed = _packed(data, geo, C)
    img = resize_batch(packed, size, "bilinear", crops, flips)
    kw["device"] = img.device

    def small(masks, name):
        if masks is None:
            return None
        m = _mask_list(masks, len(packed), name, img.device)
        if m.sizes != packed.sizes:
            raise ValueError(f"every one of {name} must have its image's size")
        return resize_batch(m, size, "nearest", crops, flips, out_dtype=torch.uint8)

    return prepare_finetune_batch(img, small(gt_masks, "gt_masks"), small(instance_masks, "instance_masks"), small(edge_masks, "edge_masks"),
                                  **kw)


def quantise_map(pred):
    """The 8-bit value of include/camo_seg_measures.h of every element: rint(clamp(pred, 0, 1) * 255) with the multiply in fp32, ties
    to even, a NaN gives 0 -> uint8."""
    p = pred.to(torch.float32)
    p = torch.where(p != p, torch.zeros_like(p), p).clamp(0.0, 1.0)
    return (p * 255.0).round().to(torch.uint8)


def _files_by_stem(folder):
    return {os.path.splitext(f)[0]: os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.lower().endswith(IMAGE_SUFFIXES)}


def detect_camouflage_directory(rg_model, image_dir, mask_dir=None, out_dir=None, batch_size=16, results_json=None, image_ids=None, **kw):
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
    "score": the instance's Sq / (255 area), "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1]}; the result also holds "results": that list."""
    from PIL import Image
    refined = _refine.refine_options(kw.get("refine")) is not None
    match = _match.match_options(kw.pop("match", None), kw.get("instances", False), mask_dir is not None, coco=True)
    if results_json is not None:
        if not isinstance(results_json, (str, os.PathLike)):
            raise ValueError(f"results_json must be a path, got {results_json!r}")
        if not kw.get("instances", False):
            raise ValueError("results_json needs instances=True: the instances are what it writes")
        kw["rle"] = True
    elif image_ids is not None:
        raise ValueError("image_ids needs results_json")
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
    if match is not None and match["gt_labels"] is not None and len(match["gt_labels"]) != len(stems):
        raise ValueError(f'match["gt_labels"] holds {len(match["gt_labels"])} maps for {len(stems)} files')
    if match is not None and match["gt_rles"] is not None and len(match["gt_rles"]) != len(stems):
        raise ValueError(f'match["gt_rles"] holds {len(match["gt_rles"])} lists for {len(stems)} files')
    coco_sizes = None
    if match is not None:
        coco = match.pop("gt_coco")
        if coco is not None:
            truth = _polygons.coco_ground_truth(coco, stems)
            match["gt_segmentations"], coco_sizes = truth["segmentations"], truth["sizes"]
            if results_json is not None and image_ids is None:
                image_ids = truth["image_ids"]
    if match is not None and match["gt_segmentations"] is not None and len(match["gt_segmentations"]) != len(stems):
        raise ValueError(f'match["gt_segmentations"] holds {len(match["gt_segmentations"])} lists for {len(stems)} files')
    if image_ids is not None and set(stems) - set(image_ids):
        raise ValueError(f"image_ids has no entry for {sorted(set(stems) - set(image_ids))[:5]}")
    results = []
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
        if match is not None and match["gt_rles"] is not None:
            out = detect_camouflage_ragged(rg_model, arrays, match=dict(match, gt_rles=match["gt_rles"][at:at + len(part)]), **kw)
        elif match is not None and match["gt_segmentations"] is not None:
            out = detect_camouflage_ragged(rg_model, arrays, match=dict(match, gt_segmentations=match["gt_segmentations"][at:at + len(part)]), **kw)
        elif match is not None:
            gt_labels = match["gt_labels"][at:at + len(part)] if match["gt_labels"] is not None else \
                _native_gt_labels([gts.image(i) for i in range(len(part))], kw.get("connectivity", 8), match["max_gt"])
            out = detect_camouflage_ragged(rg_model, arrays, match=dict(match, gt_labels=gt_labels), **kw)
        else:
            out = detect_camouflage_ragged(rg_model, arrays, **kw)
        if match is not None:
            matched += out["instance_match"]
            ap.add(out["instance_match"], [[inst["score"] for inst in r["instances"]] for r in out["instances_native"]])
        if results_json is not None:
            results += _rle.coco_results(part, out["instances_native"], out["instance_rles_native"], image_ids)
        native = out["prob_maps_native_refined" if refined else "prob_maps_native"]
        if out_dir is not None:
            for s, p in zip(part, native):
                Image.fromarray(quantise_map(p).cpu().numpy()).save(os.path.join(out_dir, s + ".png"))
        if masks is not None:
            if evaluate_at == "resized":
                small = resize_batch(gts, size, "nearest", out_dtype=torch.uint8)
                m, c = _score(list(out["prob_refined"] if refined else out["prob_maps"][:, 0]), list(small), threshold, cod, curves=True)
            else:
                m, c = _score(native, [gts.image(i) for i in range(len(part))], threshold, cod, curves=True)
            metrics += m
            cods += c or []
    if masks is not None:
        result["metrics"] = metrics
        if cod:
            result["aggregate"] = seg_measures.aggregate_cod_measures(cods)
            result["cod_metrics"] = [{k: v for k, v in c.items() if k not in ("f_curve", "e_curve")} for c in cods]
    if match is not None:
        result["instance_match"], result["instance_ap"] = matched, ap.result()
    if results_json is not None:
        with open(results_json, "w") as f:
            json.dump(results, f)
        result["results"] = results
    return result
