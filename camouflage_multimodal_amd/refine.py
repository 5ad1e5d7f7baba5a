"""Edge-aware mask refinement on MI355X (include/camo_guided.h): the step between a coarse probability map and
everything that consumes it.

The detector paints one probability per superpixel, so its mask is a mosaic whose outline is the SLIC boundary.  ``guided_filter``
(He, Sun, Tang: "Guided Image Filtering") snaps such a map to the edges of the image it came from -- box means, one small solve per
pixel, box means again, all in float64 on the device -- and ``guided_upsample`` is the second half of the fast variant: the filter's
working-size coefficients taken to every image's native size and applied to the native 8-bit pixels, in one launch for a ragged
batch.  ``detect_camouflage_batch`` / ``detect_camouflage_ragged`` run them with ``refine=``.  PARITY UNPINNED: the header's text
is the definition (restated in numpy in tests/guided_ref.py).  There is no CPU path: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, image_planes, workspace
from .resize import _ragged, upload_table

DEFAULTS = {"radius": 8, "eps": 1e-4, "guide": "rgb"}
LUMA = (0.2989, 0.5870, 0.1140)      # include/camo_canny.h step 1


def check_arguments(radius=8, eps=1e-4):
    """The ``ValueError`` of a bad setting, by name, before anything touches the device."""
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or not 1 <= radius <= _lib.GF_MAX_RADIUS:
        raise ValueError(f"radius must be an integer in [1, {_lib.GF_MAX_RADIUS}], got {radius!r}")
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or math.isnan(eps) or not _lib.GF_MIN_EPS <= eps <= _lib.GF_MAX_EPS:
        raise ValueError(f"eps must be a number in [{_lib.GF_MIN_EPS}, {_lib.GF_MAX_EPS}], got {eps!r}")


def refine_options(refine):
    """``refine`` of the detector entry points -- ``None`` / ``False`` (off), ``True`` (the defaults) or a dict with any of "radius",
    "eps", "guide" ("rgb" | "gray") -- as ``None`` or the complete dict; anything else raises ``ValueError``."""
    if refine is None or refine is False:
        return None
    if refine is True:
        return dict(DEFAULTS)
    if not isinstance(refine, dict) or set(refine) - set(DEFAULTS):
        raise ValueError(f"refine must be None, True or a dict with keys among {sorted(DEFAULTS)}, got {refine!r}")
    opt = {**DEFAULTS, **refine}
    check_arguments(opt["radius"], opt["eps"])
    if opt["guide"] not in ("rgb", "gray"):
        raise ValueError(f'refine["guide"] must be "rgb" or "gray", got {opt["guide"]!r}')
    return opt


def luma(images):
    """fp32 [N, H, W, 3] -> fp32 [N, H, W]: include/camo_canny.h's luma, 0.2989 r + 0.5870 g + 0.1140 b, in fp32 where the images are."""
    return LUMA[0] * images[..., 0] + LUMA[1] * images[..., 1] + LUMA[2] * images[..., 2]


@torch.no_grad()
def guided_filter(guide, p, radius=8, eps=1e-4, clamp=True, return_coefficients=False):
    """``camo_guided_filter``: ``guide`` fp32 [N, H, W, C] (C = 1 or 3) or [N, H, W], values meant in [0, 1]; ``p`` fp32 [N, H, W]
    (one channel of a [N, C', H, W] map is read in place through its image stride).  A single image -- ``p`` [H, W] with ``guide``
    [H, W, 3] or [H, W] -- is N = 1.  Returns ``q`` fp32 [N, H, W], the guided filter of ``p`` with windows of ``radius`` clipped at the
    image's edge and regulariser ``eps``, clamped to [0, 1] with ``clamp``; with ``return_coefficients`` (``q``, ``coef``), ``coef``
    fp32 [N, C + 1, H, W] = the mean coefficients abar_0 .. abar_{C-1}, bbar that ``guided_upsample`` consumes.  Four launches whatever
    N is, no host synchronisation; float64 between the fp32 inputs and outputs; two calls give the same bytes."""
    check_arguments(radius, eps)
    if not isinstance(guide, torch.Tensor) or not isinstance(p, torch.Tensor):
        raise ValueError("guide and p must be tensors")
    if p.dim() == 2:
        if guide.dim() not in (2, 3):
            raise ValueError(f"a single map p [H, W] needs guide [H, W, C] or [H, W], got {tuple(guide.shape)}")
        p, guide = p.unsqueeze(0), guide.unsqueeze(0)
    if guide.dim() == 3:
        guide = guide.unsqueeze(3)
    if p.dim() != 3 or guide.dim() != 4 or tuple(guide.shape[:3]) != tuple(p.shape) or p.numel() == 0:
        raise ValueError(f"need guide [N, H, W, C] or [N, H, W] and p [N, H, W] of the same N, H, W; got {tuple(guide.shape)} and {tuple(p.shape)}")
    N, H, W = p.shape
    C = int(guide.shape[3])
    if C not in (1, 3):
        raise ValueError(f"the guide must have 1 or 3 channels, got {C}")
    _lib.require_device(guide, "guide")
    _lib.require_device(p, "p")
    if guide.device != p.device:
        raise ValueError("guide and p must be on the same device")
    guide = guide.detach().to(torch.float32).contiguous()
    p, stride = image_planes(p)
    dev = p.device
    ws, nbytes = workspace("camo_guided_workspace_bytes", N, H, W, C, device=dev,
                           refuse=lambda: ValueError(f"camo_guided_filter does not support N = {N}, H = {H}, W = {W}"))
    q = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    coef = torch.empty(N, C + 1, H, W, dtype=torch.float32, device=dev) if return_coefficients else None
    call("camo_guided_filter", dev, _ptr(guide), _ptr(p), stride, N, H, W, C, int(radius), float(eps), 1 if clamp else 0, _ptr(q),
         _ptr(coef), _ptr(ws), nbytes, _stream_ptr(dev))
    return (q, coef) if return_coefficients else q


@torch.no_grad()
def guided_apply_table(coef, guide, out, table, max_dst_pixels, clamp=True):
    """``camo_guided_apply`` as it is: ``coef`` fp32 [N, C + 1, h, w], ``guide`` a uint8 device buffer, ``out`` an fp32 device buffer
    (written in place), ``table`` int64 [N, 4] rows (guide offset, H_i, W_i, out offset) -- a device tensor or nested lists; the
    kernel guards every row.  Returns the int32 [N] status tensor on the device (0 = row done, 1 = row refused, its destination
    zeroed), which nothing here reads back."""
    for t, name in ((coef, "coef"), (guide, "guide"), (out, "out")):
        _lib.require_device(t, name)
    if coef.dtype != torch.float32 or coef.dim() != 4 or coef.shape[1] not in (2, 4) or coef.numel() == 0:
        raise ValueError(f"need fp32 coef [N, C + 1, h, w] with C = 1 or 3, got {coef.dtype} {tuple(coef.shape)}")
    if guide.dtype != torch.uint8 or out.dtype != torch.float32 or guide.numel() == 0 or out.numel() == 0:
        raise ValueError(f"need a uint8 guide and an fp32 out, got {guide.dtype} and {out.dtype}")
    dev = coef.device
    if guide.device != dev or out.device != dev:
        raise ValueError("coef, guide and out must be on the same device")
    if not (guide.is_contiguous() and out.is_contiguous()):
        raise ValueError("guide and out must be contiguous buffers")
    coef = coef.detach().contiguous()
    N, _, h, w = coef.shape
    tb = upload_table(table, _lib.GF_FIELDS, dev, n=N)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    call("camo_guided_apply", dev, _ptr(coef), N, coef.shape[1] - 1, h, w, _ptr(guide), guide.numel(), _ptr(out), out.numel(), _ptr(tb),
         int(max_dst_pixels), 1 if clamp else 0, _ptr(status), _stream_ptr(dev))
    return status


@torch.no_grad()
def guided_upsample(coef, images, clamp=True):
    """The fast guided filter's second half: ``coef`` fp32 [N, C + 1, h, w] (``guided_filter``'s, taken at the working size) sampled
    bilinearly (``camo_resize``'s rule) at every pixel of N native images and applied to their own 8-bit values, q = abar . (u8 / 255)
    + bbar in float64, in ONE launch.  ``images``: anything ``resize_batch`` takes as a ragged batch -- a ``RaggedImages``, a list of
    uint8 images or a uint8 [N, H, W, C] / [N, H, W] device tensor -- with C channels.  Returns (list of N fp32 [H_i, W_i] views, the
    ONE packed buffer they are views of), like ``resize_to_sizes``."""
    if not isinstance(coef, torch.Tensor):
        raise ValueError("coef must be a tensor")
    _lib.require_device(coef, "coef")
    if coef.dtype != torch.float32 or coef.dim() != 4 or coef.shape[1] not in (2, 4) or coef.numel() == 0:
        raise ValueError(f"need fp32 coef [N, C + 1, h, w] with C = 1 or 3, got {coef.dtype} {tuple(coef.shape)}")
    data, geo, C, _ = _ragged(images, coef.device)
    if C != coef.shape[1] - 1:
        raise ValueError(f"coef is of a {coef.shape[1] - 1}-channel guide, the images have {C} channels")
    if len(geo) != coef.shape[0]:
        raise ValueError(f"coef holds {coef.shape[0]} images, the batch {len(geo)}")
    rows, at = [], 0
    for i, (o, H, W, _, _) in enumerate(geo):
        if not (1 <= H <= _lib.RSZ_MAX_SIDE and 1 <= W <= _lib.RSZ_MAX_SIDE):
            raise ValueError(f"image {i}: every side must be in [1, {_lib.RSZ_MAX_SIDE}], got {H} x {W}")
        rows.append([o, H, W, at])
        at += H * W
    buf = torch.empty(at, dtype=torch.float32, device=coef.device)
    guided_apply_table(coef, data.reshape(-1), buf, rows, max(r[1] * r[2] for r in rows), clamp)
    return [buf[r[3]:r[3] + r[1] * r[2]].view(r[1], r[2]) for r in rows], buf
