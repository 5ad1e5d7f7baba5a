"""COCO run-length masks on MI355X (include/camo_rle.h): instances out, ground truth in.

``label_runs`` runs ``camo_rle_runs`` on the label maps ``mask_instances`` writes -- (start, label) of every run along COCO's
column-major order -- and returns device tensors; ``rles_from_runs`` reads every id's COCO RLE ({"size": [H, W], "counts": str}) off
the runs on the host; ``encode_instances`` is the two together with a capacity that always holds every run.  ``decode_rles`` runs
``camo_rle_decode``: the counts of COCO annotations painted into int32 label maps on the device.  ``counts_to_string`` and
``string_to_counts`` are COCO's rleToString / rleFrString in numpy.
PARITY UNPINNED: the header's text is the definition (restated in numpy in tests/rle_ref.py).  Polygon annotations: polygons.py.  Out of scope:
``iscrowd``, IoU in the RLE domain.  There is no CPU path for the label maps: tensors that are not on a HIP device raise.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, label_map, workspace


def _counts_array(cnts, name="counts"):
    a = np.asarray(cnts)
    if a.size == 0 and a.ndim == 1:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or a.dtype.kind not in "iu" or a.dtype == np.bool_:
        raise ValueError(f"{name} must be a one-dimensional sequence of integers, got {a.dtype} {a.shape}")
    return a.astype(np.int64)


def _strings(c, lengths):
    """The strings of several count lists given back to back (``c`` int64 >= 0, ``lengths`` their sizes) in one vectorised pass."""
    lengths = np.asarray(lengths, np.int64)
    starts = np.cumsum(lengths) - lengths
    x = c.copy()
    late = np.flatnonzero(np.arange(c.size) - np.repeat(starts, lengths) > 2)      # the counts with i > 2 within their list
    x[late] -= c[late - 2]
    cols, alive = [], []
    more = np.ones(x.shape, bool)
    while more.any():
        g = x & 31
        x = x >> 5                                                   # (arithmetic: int64)
        alive.append(more)
        more = more & np.where(g & 16 != 0, x != -1, x != 0)
        cols.append(g | np.where(more, 32, 0))
    if not cols:
        return [""] * lengths.size
    chars, alive = (np.stack(cols, axis=1) + 48).astype(np.uint8), np.stack(alive, axis=1)
    text = chars[alive].tobytes().decode("ascii")
    at = np.concatenate([[0], np.cumsum(alive.sum(axis=1))])         # the first character of every count
    return [text[a:b] for a, b in zip(at[starts].tolist(), at[starts + lengths].tolist())]


def counts_to_string(cnts):
    """COCO's rleToString: count i as ``x = cnts[i]``, minus ``cnts[i - 2]`` when i > 2, in groups of five bits, low group first,
    bit 32 of a character says that another group follows, every character offset by 48.  Vectorised over the counts."""
    c = _counts_array(cnts)
    if (c < 0).any():
        raise ValueError("counts must be >= 0")
    return _strings(c, [c.size])[0]


def string_to_counts(s):
    """COCO's rleFrString, the inverse of ``counts_to_string`` -> int64 array.  A character outside the 64 of the alphabet, or a
    string that ends inside a count, raises ``ValueError``."""
    if isinstance(s, bytes):
        s = s.decode("ascii", "replace")
    if not isinstance(s, str):
        raise ValueError(f"counts must be a string, got {type(s).__name__}")
    if not s:
        return np.zeros(0, np.int64)
    try:
        b = np.frombuffer(s.encode("ascii"), np.uint8).astype(np.int64) - 48
    except UnicodeEncodeError:
        raise ValueError("counts holds a character outside COCO's alphabet") from None
    if ((b < 0) | (b > 63)).any():
        raise ValueError("counts holds a character outside COCO's alphabet")
    last = (b & 32) == 0                                             # the last group of a count
    if not last[-1]:
        raise ValueError("counts ends inside a count")
    ends = np.flatnonzero(last)
    starts = np.concatenate([[0], ends[:-1] + 1])
    length = ends - starts + 1
    if (length > 12).any():
        raise ValueError("counts holds a count of more than 12 groups")
    k = np.arange(b.size) - np.repeat(starts, length)                # a character's group number within its count
    x = np.add.reduceat((b & 31) << (5 * k), starts)
    x = np.where(b[ends] & 16 != 0, x | (np.int64(-1) << (5 * length)), x)
    out = x.copy()
    out[2::2] = np.cumsum(x[2::2])                                   # cnts[i] = x[i] + cnts[i - 2] for i > 2: two running sums,
    out[1::2] = np.cumsum(x[1::2])                                   # over the even indices from 2 and over the odd ones from 1
    return out


def _rle_counts(rle, H=None, W=None, what="rle"):
    """The int64 counts of one RLE dict ({"size": [h, w], "counts": str, bytes or a list of integers})."""
    if not isinstance(rle, dict) or "counts" not in rle or "size" not in rle:
        raise ValueError(f'{what} must be a dict with "size" and "counts", got {rle!r}')
    size = rle["size"]
    try:
        size = [int(v) for v in size]
    except (TypeError, ValueError):
        size = None
    if size is None or len(size) != 2:
        raise ValueError(f'{what}: "size" must be [h, w], got {rle["size"]!r}')
    if H is not None and size != [H, W]:
        raise ValueError(f"{what}: size {size} is not the image's {[H, W]}")
    c = rle["counts"]
    try:
        cnts = string_to_counts(c) if isinstance(c, (str, bytes)) else _counts_array(c, f'{what}: "counts"')
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    if (cnts < 0).any():
        raise ValueError(f"{what}: a count is negative")
    return cnts, size


def rle_area(rle):
    """The pixels of one RLE: the sum of its 2nd, 4th, ... counts."""
    return int(_rle_counts(rle)[0][1::2].sum())


def _check_max_runs(max_runs, n_images):
    if isinstance(max_runs, bool) or not isinstance(max_runs, numbers.Integral) or max_runs < 1:
        raise ValueError(f"max_runs must be an integer >= 1, got {max_runs!r}")
    if n_images * max_runs > _lib.RLE_MAX_ROWS:
        raise ValueError(f"max_runs = {max_runs} for {n_images} images exceeds {_lib.RLE_MAX_ROWS} rows")
    return int(max_runs)


@torch.no_grad()
def label_runs(labels, max_runs=4096):
    """``camo_rle_runs``: ``labels`` int32 [N, H, W] (or [H, W]) -> {"runs": int32 [N, max_runs, 2] = (start, label) of every
    maximal run of equal label along p = x H + y, background runs included, zero past the last, "counts": int32 [N, 2] = (the runs
    the image holds, the runs written)}, on the device, no host synchronisation."""
    labels = label_map(labels, "labels")
    N, H, W = labels.shape
    R = _check_max_runs(max_runs, N)
    _lib.require_device(labels, "labels")
    labels = labels.detach().contiguous()
    dev = labels.device
    ws, nbytes = workspace("camo_rle_runs_workspace_bytes", N, H, W, R, device=dev,
                           refuse=lambda: ValueError(f"camo_rle_runs does not support N = {N}, H = {H}, W = {W}, max_runs = {R}"))
    runs = torch.empty(N, R, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(N, 2, dtype=torch.int32, device=dev)
    call("camo_rle_runs", dev, _ptr(labels), N, H, W, R, _ptr(runs), _ptr(counts), _ptr(ws), nbytes, _stream_ptr(dev))
    return {"runs": runs, "counts": counts}


def _host_runs(runs, counts):
    """(runs [N, R, 2], counts [N, 2]) as numpy arrays; two device tensors cost the ONE host copy."""
    if isinstance(runs, torch.Tensor) and isinstance(counts, torch.Tensor) and runs.is_cuda:
        flat = torch.cat([runs.reshape(-1), counts.to(device=runs.device, dtype=runs.dtype).reshape(-1)]).cpu().numpy()      # (the one copy)
        return flat[:runs.numel()].reshape(tuple(runs.shape)), flat[runs.numel():].reshape(tuple(counts.shape))
    r = runs.cpu().numpy() if isinstance(runs, torch.Tensor) else np.asarray(runs)
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    return r, c


def rles_from_runs(runs, counts, H, W):
    """Per image {id: {"size": [H, W], "counts": str}} for every id > 0, in id order, from ``label_runs``' tensors (or arrays of their
    shapes).  An id's COCO counts are the gaps between its runs and their lengths in turn -- a leading 0 when it owns position 0, a
    last gap up to H W when it does not own the last position.  An image whose runs were not all written raises ``ValueError``."""
    r, c = _host_runs(runs, counts)
    if r.ndim == 2:
        r, c = r[None], np.reshape(c, (1, -1))
    if r.ndim != 3 or r.shape[2] != 2 or c.shape != (r.shape[0], 2):
        raise ValueError(f"need runs [N, R, 2] and counts [N, 2], got {r.shape} and {c.shape}")
    HW = int(H) * int(W)
    out = []
    for n in range(r.shape[0]):
        M, wrote = int(c[n, 0]), int(c[n, 1])
        if M > wrote:
            raise ValueError(f"image {n} holds {M} runs and {wrote} were written: call label_runs with max_runs >= {M}")
        start, label = r[n, :M, 0].astype(np.int64), r[n, :M, 1]
        length = np.diff(np.append(start, HW))
        fg = np.flatnonzero(label > 0)
        order = fg[np.argsort(label[fg], kind="stable")]              # by id, an id's runs in increasing start
        ids, s, l = label[order], start[order], length[order]
        if ids.size == 0:                                            # all background
            out.append({})
            continue
        first = np.flatnonzero(np.append(True, ids[1:] != ids[:-1]))
        gap = s - np.append(0, (s + l)[:-1])
        gap[first] = s[first]                                        # an id's first gap runs from position 0
        pairs = np.stack([gap, l], axis=1).reshape(-1)
        end = np.append(first[1:], ids.size).astype(np.int64)        # one past an id's last run
        tail = HW - (s + l)[end - 1]
        pairs = np.insert(pairs, 2 * end[tail > 0], tail[tail > 0])   # the last gap of an id that does not own the last position
        text = _strings(pairs.astype(np.int64), 2 * (end - first) + (tail > 0))      # every id's string in one pass
        out.append({int(i): {"size": [int(H), int(W)], "counts": t} for i, t in zip(ids[first].tolist(), text)})
    return out


@torch.no_grad()
def encode_instances(labels, max_runs=4096):
    """``label_runs`` and ``rles_from_runs`` together: per image {id: RLE} of ``labels`` int32 [N, H, W] (or [H, W]).  When an image
    holds more than ``max_runs`` runs the call is made once more with the capacity of the largest count, so no RLE is cut short.
    Two host copies: the counts, then the rows of ``runs`` that hold a run."""
    labels = label_map(labels, "labels")
    N, H, W = labels.shape
    out = label_runs(labels, max_runs)
    c = out["counts"].cpu().numpy()
    if (c[:, 0] > c[:, 1]).any():
        out = label_runs(labels, int(c[:, 0].max()))
        c[:, 1] = c[:, 0]                                            # (the counts of the second call, known without a copy)
    return rles_from_runs(out["runs"][:, :int(c[:, 1].max())].cpu().numpy(), c, H, W)      # only the rows that hold a run are copied


def _annotations(per_image_rles, H, W, image_numbers=None):
    """``decode_rles``' argument as (counts of all annotations back to back, offsets, images, values), int32 arrays; every
    ``ValueError`` by image and annotation."""
    for v, name in ((H, "H"), (W, "W")):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    H, W = int(H), int(W)
    if not isinstance(per_image_rles, (list, tuple)) or not per_image_rles:
        raise ValueError("per_image_rles must be a non-empty list with one list of RLEs per image")
    if image_numbers is not None and len(image_numbers) != len(per_image_rles):
        raise ValueError(f"{len(image_numbers)} image numbers for {len(per_image_rles)} images")
    chunks, off, images, values = [], [0], [], []
    for i, anns in enumerate(per_image_rles):
        n = i if image_numbers is None else image_numbers[i]
        if isinstance(anns, dict) and "counts" not in anns:
            anns = [(rle, v) for v, rle in anns.items()]              # {id: rle}, as encode_instances returns it
        if not isinstance(anns, (list, tuple)):
            raise ValueError(f"image {n}: need a list of RLE dicts or (rle, value) pairs, got {type(anns).__name__}")
        for k, ann in enumerate(anns):
            what = f"image {n}, annotation {k}"
            rle, value = (ann[0], ann[1]) if isinstance(ann, (list, tuple)) and len(ann) == 2 else (ann, k + 1)
            if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not 1 <= value <= 2 ** 31 - 1:
                raise ValueError(f"{what}: the value must be an integer in [1, 2^31 - 1], got {value!r}")
            cnts, _ = _rle_counts(rle, H, W, what)
            if int(cnts.sum()) != H * W:
                raise ValueError(f"{what}: the counts sum to {int(cnts.sum())}, the image has {H * W} pixels")
            chunks.append(cnts)
            off.append(off[-1] + cnts.size)
            images.append(i)
            values.append(int(value))
    if len(images) > _lib.RLE_MAX_ANNOTATIONS:
        raise ValueError(f"{len(images)} annotations exceed {_lib.RLE_MAX_ANNOTATIONS}")
    if off[-1] > _lib.RLE_MAX_COUNTS:
        raise ValueError(f"{off[-1]} counts exceed {_lib.RLE_MAX_COUNTS}")
    cnts = np.concatenate(chunks).astype(np.int32) if chunks else np.zeros(0, np.int32)
    return cnts, np.asarray(off, np.int32), np.asarray(images, np.int32), np.asarray(values, np.int32)


@torch.no_grad()
def decode_counts(cnts, ann_off, ann_image, ann_value, N, H, W, device="cuda"):
    """``camo_rle_decode`` on host arrays: the counts of A annotations back to back (int32 [total]), ``ann_off`` [A + 1]
    non-decreasing from 0 to total, ``ann_image`` [A] and ``ann_value`` [A] -> (labels int32 [N, H, W], ann_sum int64 [A]) on
    ``device``, no host synchronisation after the upload.  The arrays go up in ONE copy.  ``ann_sum`` is the sum of an annotation's
    counts, -1 for one with a negative count, an image outside the batch or a value below 1, which paints nothing."""
    cnts, ann_off = np.asarray(cnts, np.int32).reshape(-1), np.asarray(ann_off, np.int32).reshape(-1)
    ann_image, ann_value = np.asarray(ann_image, np.int32).reshape(-1), np.asarray(ann_value, np.int32).reshape(-1)
    A, total = ann_image.size, cnts.size
    for v, name in ((N, "N"), (H, "H"), (W, "W")):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    if not 1 <= A <= _lib.RLE_MAX_ANNOTATIONS:
        raise ValueError(f"need 1 .. {_lib.RLE_MAX_ANNOTATIONS} annotations, got {A}")
    if ann_value.size != A or ann_off.size != A + 1:
        raise ValueError(f"need ann_off of {A + 1} and ann_value of {A} integers, got {ann_off.size} and {ann_value.size}")
    if total > _lib.RLE_MAX_COUNTS:
        raise ValueError(f"{total} counts exceed {_lib.RLE_MAX_COUNTS}")
    if ann_off[0] != 0 or ann_off[-1] != total or (np.diff(ann_off) < 0).any():
        raise ValueError(f"ann_off must be non-decreasing from 0 to the number of counts, {total}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.CamoError(f"the label maps are painted on {dev}: camo_rle_decode runs as HIP kernels on an MI355X and has no CPU fallback")
    ws, nbytes = workspace("camo_rle_decode_workspace_bytes", int(N), int(H), int(W), A, total, device=dev,
                           refuse=lambda: ValueError(f"camo_rle_decode does not support N = {N}, H = {H}, W = {W}, {A} annotations, {total} counts"))
    up = torch.from_numpy(np.concatenate([ann_off, ann_image, ann_value, cnts])).to(dev)      # (the one copy)
    d_off, d_img, d_val, d_cnt = up[:A + 1], up[A + 1:2 * A + 1], up[2 * A + 1:3 * A + 1], up[3 * A + 1:]
    labels = torch.empty(int(N), int(H), int(W), dtype=torch.int32, device=dev)
    ann_sum = torch.empty(A, dtype=torch.int64, device=dev)
    call("camo_rle_decode", dev, _ptr(d_cnt) if total else None, total, _ptr(d_off), _ptr(d_img), _ptr(d_val), A, int(N), int(H), int(W),
         _ptr(labels), _ptr(ann_sum), _ptr(ws), nbytes, _stream_ptr(dev))
    return labels, ann_sum


@torch.no_grad()
def decode_rles(per_image_rles, H, W, device="cuda", image_numbers=None):
    """``camo_rle_decode``: ``per_image_rles`` -- per image a list of RLE dicts or (rle, value) pairs, or the {id: rle} dict
    ``encode_instances`` returns -- painted into ``labels`` int32 [N, H, W] on ``device``.  Values default to 1 .. K in list order;
    where annotations overlap the largest value wins, so with the default values the later one.  A ``size`` other than [H, W] or counts
    that do not sum to H W raise ``ValueError`` naming the image and the annotation, on the host before anything is uploaded
    (``image_numbers``: the numbers the messages give the images, when the list is a part of a larger one)."""
    cnts, off, images, values = _annotations(per_image_rles, H, W, image_numbers)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.CamoError(f"the label maps are painted on {dev}: camo_rle_decode runs as HIP kernels on an MI355X and has no CPU fallback")
    N = len(per_image_rles)
    if images.size == 0:                                             # no annotation at all: nothing to paint
        return torch.zeros(N, int(H), int(W), dtype=torch.int32, device=dev)
    return decode_counts(cnts, off, images, values, N, int(H), int(W), dev)[0]


def rle_options(rle, instances=True):
    """The pipeline's ``rle`` keyword as a bool; the ``ValueError`` of a bad one by name."""
    if not isinstance(rle, bool):
        raise ValueError(f"rle must be True or False, got {rle!r}")
    if rle and not instances:
        raise ValueError("rle needs instances=True: the instances are what it encodes")
    return rle


def coco_results(stems, instances, rles, image_ids=None, category_id=1):
    """COCO results entries of some images: ``instances`` per image the records of ``instance_records``, ``rles`` per image
    ``encode_instances``' {id: rle}.  Per instance {"image_id": the stem or ``image_ids[stem]``, "category_id", "segmentation": the
    RLE, "score": the record's Sq / (255 area), "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1]}."""
    out = []
    for stem, rec, enc in zip(stems, instances, rles):
        for inst in rec["instances"]:
            x0, y0, x1, y1 = inst["box"]
            out.append({"image_id": stem if image_ids is None else image_ids[stem], "category_id": category_id,
                        "segmentation": enc[inst["id"]], "score": inst["score"], "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1]})
    return out
