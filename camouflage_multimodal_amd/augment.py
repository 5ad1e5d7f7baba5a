"""Rotation and colour augmentation on the device (include/camo_augment.h).

Camouflaged-object training recipes augment with a flip, a crop, a rotation of +-15 degrees and PIL's four ``ImageEnhance``
operations.  ``random_cod_augmentation`` draws all of that on the host from a seed, ``affine_rows`` turns a crop, a flip, an angle
and a zoom per image into the integers of the inverse map, and ``augment_batch`` runs ``camo_augment`` over a ragged batch: the warp
in ONE launch, the warp and the four enhancements in three.  ``prepare_finetune_batch_ragged(augment=...)`` of rg_finetune.py sends
the image through it bilinear with the factors and every mask nearest with the same maps.  PARITY UNPINNED: the header's text defines
the result in exact integers (tests/augment_ref.py restates it; PIL agrees within a grey level per enhancement).  There is no CPU
path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, workspace
from .resize import _ragged, check_filter, check_out_dtype, check_size, draw_crop, upload_table

FILTERS = {"nearest": _lib.RSZ_NEAREST, "bilinear": _lib.RSZ_BILINEAR}
BORDERS = {"constant": 0, "replicate": 1}
ROW_FIELDS = 12     # what affine_rows gives per image: fields 6 .. 17 of the header's table
_ONE = 1 << _lib.AUG_FRAC_BITS


def _fill_word(fill, n):
    """``fill`` -- one byte value for every channel, or a sequence of up to four -- as the header's field 17, N times."""
    vals = [int(fill)] * 4 if np.isscalar(fill) else [int(v) for v in fill]
    if not 1 <= len(vals) <= 4 or any(not 0 <= v <= 255 for v in vals):
        raise ValueError(f"fill must be a byte value or up to four of them, got {fill!r}")
    return [sum(v << (8 * c) for c, v in enumerate(vals))] * n


def affine_rows(sizes, size, crops=None, flips=None, angles=None, zooms=None, border="constant", fill=0):
    """The map of ``camo_augment`` for images of ``sizes`` [(H, W), ...] and a destination ``size`` = (Ho, Wo): per image the twelve
    integers (clip_y0, clip_x0, clip_h, clip_w, a00, a01, b0, a10, a11, b1, border, fill), fields 6 .. 17 of the header's table.
    Host float64: with u = dx + 1/2 - Wo/2 and v = dy + 1/2 - Ho/2 the source point of destination pixel (dy, dx) is
    box centre + R(angle) . diag(cw / Wo, ch / Ho) . Flip . (u, v) / zoom in continuous coordinates, the box being ``crops[i]`` =
    (y0, x0, h, w) (default: the whole image); ``flips[i]`` bit 0 mirrors columns and bit 1 rows; ``angles`` are degrees.
    a_ij = rint(m_ij 2^15), b0 = rint((x0 + cw/2 - 1/2 - m00 Wo/2 - m01 Ho/2) 2^16), likewise b1.  At angle 0 and zoom 1, with
    cw 2^15 / Wo an integer, these are exactly ``camo_resize``'s bilinear taps.  ``border``: "constant" (taps outside the whole IMAGE
    read ``fill``, a byte value or one per channel) or "replicate" (the CROP's edge is repeated, as ``resize_batch`` does)."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    N = len(sizes)
    Ho, Wo = (int(v) for v in size)
    if border not in BORDERS:
        raise ValueError(f"border must be one of {sorted(BORDERS)}, got {border!r}")
    check_size((Ho, Wo))
    crops = [(0, 0, h, w) for h, w in sizes] if crops is None else [tuple(int(v) for v in c) for c in crops]
    flips = [0] * N if flips is None else [int(f) for f in flips]
    angles = [0.0] * N if angles is None else [float(a) for a in angles]
    zooms = [1.0] * N if zooms is None else [float(z) for z in zooms]
    if not (len(crops) == len(flips) == len(angles) == len(zooms) == N) or any(len(c) != 4 for c in crops):
        raise ValueError(f"need {N} crops (y0, x0, h, w), flips, angles and zooms, got {len(crops)}, {len(flips)}, {len(angles)} and {len(zooms)}")
    fills = _fill_word(fill, N)
    rows = []
    for i, ((H, W), (y0, x0, ch, cw), f, ang, z) in enumerate(zip(sizes, crops, flips, angles, zooms)):
        if ch < 1 or cw < 1 or y0 < 0 or x0 < 0 or y0 + ch > H or x0 + cw > W:
            raise ValueError(f"image {i}: the crop (y0, x0, h, w) = {(y0, x0, ch, cw)} does not lie inside the {H} x {W} image")
        if not 0 <= f <= 3:
            raise ValueError(f"image {i}: flip must be in 0..3, got {f}")
        if not (z > 0.0 and math.isfinite(z) and math.isfinite(ang)):
            raise ValueError(f"image {i}: need a finite angle and a zoom > 0, got {ang} and {z}")
        t = math.radians(ang)
        co, si = (1.0, 0.0) if ang == 0.0 else (math.cos(t), math.sin(t))
        sx, sy = (cw / Wo) * (-1.0 if f & 1 else 1.0) / z, (ch / Ho) * (-1.0 if f & 2 else 1.0) / z
        m00, m01, m10, m11 = co * sx, -si * sy, si * sx, co * sy
        b0 = (x0 + cw / 2 - 0.5 - m00 * Wo / 2 - m01 * Ho / 2) * _ONE
        b1 = (y0 + ch / 2 - 0.5 - m10 * Wo / 2 - m11 * Ho / 2) * _ONE
        clip = (0, 0, H, W) if border == "constant" else (y0, x0, ch, cw)
        rows.append([*clip, *(int(np.rint(m * (_ONE // 2))) for m in (m00, m01)), int(np.rint(b0)),
                     *(int(np.rint(m * (_ONE // 2))) for m in (m10, m11)), int(np.rint(b1)), BORDERS[border], fills[i]])
    return rows


def _uniform_q8(rs, rng):
    return _lib.AUG_MAX_FACTOR // 4 if rng is None else int(min(max(np.rint(rs.uniform(rng[0], rng[1]) * 256), 0), _lib.AUG_MAX_FACTOR))


def random_cod_augmentation(sizes, size=(256, 256), seed=0, rotate_p=0.2, max_angle=15.0, brightness=(0.5, 1.5), contrast=(0.5, 1.5),
                            colour=(0.0, 2.0), sharpness=(0.0, 3.0), scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5):
    """The augmentation of SINet-V2's loader for images of ``sizes`` [(H, W), ...]: host only, driven by
    ``numpy.random.RandomState(seed)``, so the same seed gives the same dict.  Per image a RandomResizedCrop box (up to ten draws of an
    area fraction in ``scale`` and an aspect ratio log-uniform in ``ratio``, else the whole image), a column flip with probability
    ``flip_p``, with probability ``rotate_p`` an angle uniform in +-``max_angle`` degrees (else 0), and one factor uniform in each of
    the four ranges, as Q8 integers (256 = unchanged, at most 1024).  A range that is ``None`` leaves its factor at 256; all four
    ``None`` give ``"factors": None`` -- no enhancement.  Returns {"crops", "flips", "angles", "factors"}; ``size`` is where the
    batch will go and takes no part in the draws."""
    rs = np.random.RandomState(seed)
    ranges = (brightness, contrast, colour, sharpness)
    crops, flips, angles, factors = [], [], [], []
    for H, W in sizes:
        crops.append(draw_crop(rs, H, W, scale, ratio))
        flips.append(1 if rs.uniform() < flip_p else 0)
        turn, angle = rs.uniform() < rotate_p, float(rs.uniform(-max_angle, max_angle))
        angles.append(angle if turn else 0.0)
        factors.append(tuple(_uniform_q8(rs, r) for r in ranges))
    return {"crops": crops, "flips": flips, "angles": angles, "factors": None if all(r is None for r in ranges) else factors}


def check_rows(table, channels, src_elems, enhance):
    """The row conditions of include/camo_augment.h on host integers: a bad row raises ``ValueError`` (the kernel would refuse it)."""
    S = _lib.RSZ_MAX_SIDE
    for i, r in enumerate(table):
        so, sh, sw, srs, sps, scs, y0, x0, ch, cw, a00, a01, b0, a10, a11, b1, border, fill, kb, kc, ks, kh, r0, r1 = (int(v) for v in r)
        if not all(1 <= v <= S for v in (sh, sw, ch, cw)):
            raise ValueError(f"image {i}: every side must be in [1, {S}]: source {sh} x {sw}, clip box {ch} x {cw}")
        if y0 < 0 or x0 < 0 or y0 + ch > sh or x0 + cw > sw:
            raise ValueError(f"image {i}: the clip box (y0, x0, h, w) = {(y0, x0, ch, cw)} does not lie inside the {sh} x {sw} image")
        if min(srs, sps, scs) < 1 or so < 0 or so + (sh - 1) * srs + (sw - 1) * sps + (channels - 1) * scs >= src_elems:
            raise ValueError(f"image {i}: the source footprint leaves the source buffer")
        if max(abs(a00), abs(a01), abs(a10), abs(a11)) > 1 << 30 or max(abs(b0), abs(b1)) > 1 << 46:
            raise ValueError(f"image {i}: the map leaves |a| <= 2^30, |b| <= 2^46")
        if border not in (0, 1) or not 0 <= fill < 1 << 32 or r0 != 0 or r1 != 0:
            raise ValueError(f"image {i}: border must be 0 or 1, fill in [0, 2^32) and the reserved fields zero")
        if enhance and not all(0 <= k <= _lib.AUG_MAX_FACTOR for k in (kb, kc, ks, kh)):
            raise ValueError(f"image {i}: every factor must be in [0, {_lib.AUG_MAX_FACTOR}] (Q8), got {(kb, kc, ks, kh)}")


@torch.no_grad()
def augment_table(src, table, channels, size, filter="bilinear", enhance=False, out_dtype=torch.float32, src_elems=None):
    """``camo_augment`` as it is: ``src`` a uint8 device tensor whose storage from ``data_ptr()`` on holds ``src_elems`` bytes
    (default ``numel()``), ``table`` int64 [N, 24] -- a device tensor is used unchecked (the kernel guards every row), anything else is
    checked with ``check_rows`` and uploaded.  Returns (dst [N, Ho, Wo, C] of ``out_dtype``, the int32 [N] status tensor on the device,
    which nothing here reads back)."""
    check_filter(filter, FILTERS)
    check_out_dtype(out_dtype)
    return _augment(src, table, channels, check_size(size), filter, enhance, out_dtype, src_elems)


def _augment(src, table, channels, size, filter, enhance, out_dtype, src_elems=None):
    """``augment_table`` past the checks of ``size``, ``filter`` and ``out_dtype``, which ``augment_batch`` has made by then."""
    Ho, Wo = size
    C, enhance = int(channels), bool(enhance)
    if enhance and C != 3:
        raise ValueError(f"the enhancements need images with 3 channels, got {C}")
    _lib.require_device(src, "src")
    if src.dtype != torch.uint8:
        raise ValueError(f"src must be uint8, got {src.dtype}")
    dev = src.device
    src_elems = int(src.numel() if src_elems is None else src_elems)

    def check(rows):
        if not rows or any(len(r) != _lib.AUG_FIELDS for r in rows):
            raise ValueError(f"need a table [N, {_lib.AUG_FIELDS}]")
        check_rows(rows, C, src_elems, enhance)

    tb = upload_table(table, _lib.AUG_FIELDS, dev, check)
    N = tb.shape[0]
    dst = torch.empty((N, Ho, Wo, C), dtype=out_dtype, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    ws, need = workspace("camo_augment_workspace_bytes", N, Ho, Wo, C, int(enhance), device=dev, refuse=False)      # (the warp alone needs none)
    call("camo_augment", dev, _ptr(src), src_elems, _ptr(dst), _lib.RSZ_F32 if out_dtype == torch.float32 else _lib.RSZ_U8, _ptr(tb), N, C, Ho, Wo,
         FILTERS[filter], int(enhance), _ptr(status), _ptr(ws), need, _stream_ptr(dev))
    return dst, status


@torch.no_grad()
def augment_batch(images, size=(256, 256), rows=None, factors=None, filter="bilinear", out_dtype=torch.float32):
    """``images`` -- whatever ``resize_batch`` takes: a ``RaggedImages``, a list of uint8 images or a uint8 [N, H, W, C] / [N, H, W]
    device tensor -- through the maps ``rows`` (``affine_rows``' twelve integers per image; default: the whole image resized with its
    edge repeated, which is ``resize_batch``) to ``size`` = (Ho, Wo): fp32 [N, Ho, Wo, C] in [0, 1], or uint8 with
    ``out_dtype=torch.uint8``; images given as [H, W] come back [N, Ho, Wo].  ``factors``: N tuples (brightness, contrast, colour,
    sharpness) of Q8 integers in [0, 1024] -- the four enhancements after the warp, 3 channels only; ``None``: the warp alone, ONE
    launch.  ``filter``: "nearest" or "bilinear"."""
    check_out_dtype(out_dtype)
    check_filter(filter, FILTERS)
    Ho, Wo = check_size(size)
    data, geo, C, squeeze = _ragged(images)
    N = len(geo)
    if rows is None:
        rows = affine_rows([(g[1], g[2]) for g in geo], (Ho, Wo), border="replicate")
    rows = [[int(v) for v in r] for r in rows]
    if len(rows) != N or any(len(r) != ROW_FIELDS for r in rows):
        raise ValueError(f"need {N} rows of {ROW_FIELDS} integers (affine_rows), got {len(rows)}")
    if factors is None:
        ks = [(0, 0, 0, 0)] * N
    else:
        ks = [tuple(int(v) for v in k) for k in factors]
        if len(ks) != N or any(len(k) != 4 for k in ks):
            raise ValueError(f"need {N} factors (brightness, contrast, colour, sharpness), got {len(ks)}")
        if C != 3:
            raise ValueError(f"factors need images with 3 channels, got {C}")
    table = [[o, h, w, rs, ps, 1, *r, *k, 0, 0] for (o, h, w, rs, ps), r, k in zip(geo, rows, ks)]
    out, _ = _augment(data, table, C, (Ho, Wo), filter, factors is not None, out_dtype)
    return out[..., 0] if squeeze else out
