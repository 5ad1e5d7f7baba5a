"""Resize on the device: mixed-size images in, native-size masks out (include/camo_resize.h).

The data of this project are 8-bit files, each of its own size; the model works at one fixed size and the benchmark tables are
scored at each ground truth's own size.  ``pack_images`` puts a list of uint8 images into one device buffer, ``resize_batch``
resamples them -- with a crop box and a flip per image -- to a fixed fp32 batch in ONE launch of ``camo_resize``, and
``resize_to_sizes`` takes fp32 maps back to ragged native sizes in one launch; ``random_resized_crops`` draws the boxes and flips
of an augmentation (``draw_crop``, one box; with ``check_size``, ``check_filter``, ``check_out_dtype`` and ``upload_table`` what augment.py
and refine.py share with this module).  This module is the header's binding and imports nothing but it: what runs on top -- the entry points for
images of mixed sizes and for a folder of files -- is in pipeline.py, and the fine-tune preparation for mixed sizes in
rg_finetune.py.  PARITY UNPINNED: cv2 and skimage are absent, so the header's text defines the filters (exact integer arithmetic;
tests/resize_ref.py restates it).  There is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call

FILTERS = {"nearest": _lib.RSZ_NEAREST, "bilinear": _lib.RSZ_BILINEAR, "area": _lib.RSZ_AREA}


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


def check_size(size):
    """``size`` = (Ho, Wo) as two integers, each within [1, RSZ_MAX_SIDE]."""
    Ho, Wo = (int(v) for v in size)
    if not (1 <= Ho <= _lib.RSZ_MAX_SIDE and 1 <= Wo <= _lib.RSZ_MAX_SIDE):
        raise ValueError(f"size must be within [1, {_lib.RSZ_MAX_SIDE}] a side, got {(Ho, Wo)}")
    return Ho, Wo


def check_filter(filter, filters):
    """``filter`` against a module's own ``FILTERS``."""
    if filter not in filters:
        raise ValueError(f"filter must be one of {sorted(filters)}, got {filter!r}")


def check_out_dtype(out_dtype):
    if out_dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")


def upload_table(table, fields, device, check=None, n=None):
    """The int64 [N, ``fields``] table of a ragged call on ``device``: a device tensor is used unchecked (the kernel guards every
    row), anything else goes through ``check(rows)``, the caller's row conditions on host integers, and is uploaded; without a
    checker a host tensor goes up as it is.  ``n``: the N the caller knows."""
    if isinstance(table, torch.Tensor) and (table.is_cuda or check is None):
        tb = table.to(device=device, dtype=torch.int64).contiguous()
    else:
        rows = table.tolist() if isinstance(table, (torch.Tensor, np.ndarray)) else [list(r) for r in table]
        if check is not None:
            check(rows)
        tb = torch.tensor(rows, dtype=torch.int64).to(device)
    if tb.dim() != 2 or tb.shape[1] != fields or tb.shape[0] == 0 or (n is not None and tb.shape[0] != n):
        raise ValueError(f"need a table [{'N' if n is None else n}, {fields}], got {tuple(tb.shape)}")
    return tb


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
    check_filter(filter, FILTERS)
    dev = src.device
    if dst.device != dev:
        raise ValueError("src and dst must be on the same device")
    src_elems = int(src.numel() if src_elems is None else src_elems)
    dst_elems = int(dst.numel() if dst_elems is None else dst_elems)
    if max_dst_pixels is None and isinstance(table, torch.Tensor) and table.is_cuda:
        raise ValueError("a device table needs max_dst_pixels")

    def check(rows):
        nonlocal max_dst_pixels
        if max_dst_pixels is None:
            max_dst_pixels = max(int(r[12]) * int(r[13]) for r in rows)
        check_table(rows, channels, src_elems, dst_elems, int(max_dst_pixels))

    tb = upload_table(table, _lib.RSZ_FIELDS, dev, check)
    N = tb.shape[0]
    status = torch.empty(N, dtype=torch.int32, device=dev)
    call("camo_resize", dev, _ptr(src), src_elems, _type_of(src, "src"), _ptr(dst), dst_elems, _type_of(dst, "dst"), _ptr(tb), N,
         int(channels), FILTERS[filter], int(max_dst_pixels), _ptr(status), _stream_ptr(dev))
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
    check_out_dtype(out_dtype)
    Ho, Wo = (int(v) for v in size)
    data, geo, C, squeeze = _ragged(images)
    crops, flips = _boxes(crops, flips, geo)
    rows = [[o, h, w, rs, ps, 1, y0, x0, ch, cw, f, i * Ho * Wo * C, Ho, Wo, Wo * C, C, 1, 0]
            for i, ((o, h, w, rs, ps), (y0, x0, ch, cw), f) in enumerate(zip(geo, crops, flips))]
    check_size((Ho, Wo))                                     # (the images' and the boxes' own errors come first)
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


def draw_crop(rs, H, W, scale, ratio):
    """One RandomResizedCrop box (y0, x0, h, w) of an H x W image from the ``RandomState`` ``rs``: up to ten draws of an area
    fraction in ``scale`` and an aspect ratio (w / h) log-uniform in ``ratio``, two draws each; the first box that fits is placed
    with two draws more; after ten rejected draws the box is the whole image."""
    H, W = int(H), int(W)
    for _ in range(10):
        area = H * W * rs.uniform(scale[0], scale[1])
        aspect = math.exp(rs.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return int(rs.randint(0, H - h + 1)), int(rs.randint(0, W - w + 1)), h, w
    return 0, 0, H, W


def random_resized_crops(sizes, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=0):
    """The boxes and flips of a RandomResizedCrop + RandomHorizontalFlip for images of ``sizes`` [(H, W), ...]: host only, driven by
    ``numpy.random.RandomState(seed)``, so the same seed gives the same list.  Per image up to ten draws of an area fraction in
    ``scale`` and an aspect ratio (w / h) log-uniform in ``ratio``; the first box that fits is placed uniformly inside the image;
    after ten rejected draws the box is the whole image.  Returns (crops [(y0, x0, h, w)], flips [0 or 1: mirror the columns])."""
    rs = np.random.RandomState(seed)
    crops, flips = [], []
    for H, W in sizes:
        crops.append(draw_crop(rs, H, W, scale, ratio))
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
