"""Touching objects split on MI355X (include/camo_split.h): one connected component of the mask that holds two
animals becomes two instances.

``mask_instances`` finds objects as connected components, so two objects that touch, or that one superpixel bridges, are one
instance.  ``split_instances`` runs ``camo_split_instances`` on a label map -- the exact squared distance to the background, the
cores above ``ratio`` of each id's largest distance, every pixel of an id with two cores or more to the core of its own id with the
nearest core pixel -- and returns device tensors; ``split_records`` takes the ratios from the integers on the host;
``split_detected`` is the two together with a table that always holds every instance, for the pipeline; ``split_options`` is the
pipeline's ``split`` keyword.  ``merge_parts`` runs ``camo_split_merge`` (include/camo_split_merge.h) on a part map of
either growth: a part whose best pass to a higher part is nearly as high as its own peak is joined to it, so a lobe that one level
set cut off its body goes back while a real neck stays cut; ``split_instances(..., merge=)`` is the two calls in a row.  With
``growth="geodesic"`` (include/camo_split_geo.h) the last step measures the distance
along paths INSIDE the id, so every part is one connected piece -- what a coiled or curled animal needs.
PARITY UNPINNED: the header's text is the definition (restated in numpy in tests/split_ref.py).  There is no CPU path: tensors
that are not on a HIP device raise.
"""
from __future__ import annotations

import numbers

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call, image_planes, label_map, workspace
from .instances import instance_records

RATIO = (7, 10)
OPTIONS = {"ratio": RATIO, "min_core": 0, "max_split": 4, "max_instances": 64}
GROWTHS = ("euclidean", "geodesic")
MERGE = (4, 5)


def _integer(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def check_arguments(ratio=RATIO, min_core=0, max_split=4, max_instances=64, n_images=1):
    """The ``ValueError`` of every bad setting, by name, before anything touches the device.  -> (num, den) of ``ratio``."""
    if not isinstance(ratio, (tuple, list)) or len(ratio) != 2 or not all(_integer(v) for v in ratio) or \
            not 0 < ratio[0] < ratio[1] <= _lib.SPLIT_MAX_DEN:
        raise ValueError(f"ratio must be a pair of integers (num, den) with 0 < num < den <= {_lib.SPLIT_MAX_DEN}, got {ratio!r}")
    if not _integer(min_core) or min_core < 0:
        raise ValueError(f"min_core must be an integer >= 0, got {min_core!r}")
    if not _integer(max_split) or not 1 <= max_split <= _lib.SPLIT_MAX_SPLIT:
        raise ValueError(f"max_split must be an integer in [1, {_lib.SPLIT_MAX_SPLIT}], got {max_split!r}")
    if not _integer(max_instances) or max_instances < 1:
        raise ValueError(f"max_instances must be an integer >= 1, got {max_instances!r}")
    if n_images * max_instances > _lib.INST_MAX_ROWS:
        raise ValueError(f"max_instances = {max_instances} for {n_images} images exceeds {_lib.INST_MAX_ROWS} table rows")
    return int(ratio[0]), int(ratio[1])


def check_merge(merge=MERGE):
    """The ``ValueError`` of a bad ``merge``, by name.  -> (num, den)."""
    if not isinstance(merge, (tuple, list)) or len(merge) != 2 or not all(_integer(v) for v in merge) or \
            not 0 < merge[0] <= merge[1] <= _lib.SPLIT_MAX_DEN:
        raise ValueError(f"merge must be a pair of integers (num, den) with 0 < num <= den <= {_lib.SPLIT_MAX_DEN}, got {merge!r}")
    return int(merge[0]), int(merge[1])


def check_growth(growth="euclidean", rounds=None):
    """The ``ValueError`` of a bad ``growth`` or ``rounds``, by name."""
    if growth not in GROWTHS:
        raise ValueError(f'growth must be "euclidean" or "geodesic", got {growth!r}')
    if rounds is not None and (not _integer(rounds) or not 1 <= rounds <= _lib.SPLIT_GEO_MAX_ROUNDS):
        raise ValueError(f"rounds must be None or an integer in [1, {_lib.SPLIT_GEO_MAX_ROUNDS}], got {rounds!r}")
    if rounds is not None and growth != "geodesic":
        raise ValueError(f'rounds belongs to growth="geodesic", got growth={growth!r}')


@torch.no_grad()
def split_instances(labels, pred=None, ratio=RATIO, min_core=0, max_split=4, max_instances=64, growth="euclidean", rounds=None, merge=None):
    """``camo_split_instances``: ``labels`` int32 [N, H, W] (or [H, W]), 0 on background and an id in 1 .. 1024 per component
    (``mask_instances``' "labels"); ``pred``: ``None``, or the fp32 [N, H, W] probability the labels came from (one channel of a
    [N, C, H, W] map is read in place), for the table's Sq -> {"labels": int32 [N, H, W], the new ids 1 .. K' in input-id order, the
    parts of one id in the reading order of their cores' first pixels; "table": int64 [N, max_instances, 8] = ``mask_instances``'
    row of every new id (Sq 0 without ``pred``); "counts": int32 [N, 4] = (K', ids split, cores dropped as smaller than ``min_core``,
    qualifying ids left whole because ``max_split`` were split before them)}, all on the device, no host synchronisation.  A pixel
    is a core pixel when its squared distance to the background exceeds (num / den)^2 of its id's largest, ``ratio`` = (num, den).

    ``growth="geodesic"`` runs ``camo_split_instances_geodesic`` instead: a pixel goes to the core that the cheapest 8-neighbour path
    inside its id reaches (5 a straight step, 7 a diagonal one, a tie to the core first in reading order), so every part is connected
    and contains its core.  The growth runs in rounds of one launch each; ``rounds`` (default: tiles_x + tiles_y of 32 x 32 tiles,
    enough for every path that is monotone in both axes) are enqueued, then "pending" is read -- ONE HOST SYNCHRONISATION, which the
    Euclidean path does not have -- and ``camo_split_geodesic_resume`` runs twice the rounds again until no image has a tile left
    to grow, so the result is the header's definition for any content.  The dict then also holds "rounds": the rounds run in all.

    ``merge`` -- ``None`` (no launch more, no byte or key changed) or a pair (num, den) -- runs ``merge_parts`` on the labels the split
    leaves, after the geodesic growth has ended: "labels" and "table" are then the merged ones, "counts" stays the splitter's, and
    "merge_counts" int32 [N, 4] is ``merge_parts``' "counts"."""
    if merge is not None:
        merge = check_merge(merge)
    out = _split(labels, pred, ratio, min_core, max_split, max_instances, growth, rounds)
    if merge is None:
        return out
    merged = merge_parts(labels, out["labels"], pred, merge, max_instances)
    out.update({"labels": merged["labels"], "table": merged["table"], "merge_counts": merged["counts"]})
    return out


def _maps(labels, pred):
    """(``labels`` as int32 [N, H, W], ``pred`` as [N, H, W] or ``None``), the ``ValueError`` of anything else by name."""
    labels = label_map(labels, "labels")
    N, H, W = labels.shape
    if pred is not None:
        if not isinstance(pred, torch.Tensor):
            raise ValueError("pred must be a tensor or None")
        if pred.dim() == 2:
            pred = pred.unsqueeze(0)
        if tuple(pred.shape) != (N, H, W):
            raise ValueError(f"need pred of labels' shape {(N, H, W)}, got {tuple(pred.shape)}")
    return labels, pred


def _planes(labels, pred):
    """The two on the device as the library reads them -> (labels contiguous, pred or ``None``, its image stride)."""
    _lib.require_device(labels, "labels")
    labels = labels.detach().contiguous()
    stride = 0
    if pred is not None:
        _lib.require_device(pred, "pred")
        pred, stride = image_planes(pred)
    return labels, pred, stride


def _split(labels, pred, ratio, min_core, max_split, max_instances, growth, rounds):
    labels, pred = _maps(labels, pred)
    N, H, W = labels.shape
    num, den = check_arguments(ratio, min_core, max_split, max_instances, N)
    check_growth(growth, rounds)
    labels, pred, stride = _planes(labels, pred)
    dev = labels.device
    geodesic = growth == "geodesic"
    ws, nbytes = workspace("camo_split_geodesic_workspace_bytes" if geodesic else "camo_split_workspace_bytes", N, H, W, int(max_split), device=dev,
                           refuse=lambda: ValueError(f"camo_split_instances does not support N = {N}, H = {H}, W = {W} (a side is at most {_lib.SEG_WF_MAX_SIDE})"))
    out = torch.empty_like(labels)
    table = torch.empty(N, int(max_instances), _lib.INST_FIELDS, dtype=torch.int64, device=dev)
    counts = torch.empty(N, _lib.SPLIT_COUNTS, dtype=torch.int32, device=dev)
    args = (_ptr(labels), None if pred is None else _ptr(pred), stride, N, H, W, num, den, int(min_core), int(max_split), int(max_instances), _ptr(out),
            _ptr(table), _ptr(counts), _ptr(ws), nbytes)
    if not geodesic:
        call("camo_split_instances", dev, *args, _stream_ptr(dev))
        return {"labels": out, "table": table, "counts": counts}
    T = _lib.SPLIT_GEO_TILE
    step = int(rounds) if rounds is not None else min(-(-H // T) + -(-W // T), _lib.SPLIT_GEO_MAX_ROUNDS)
    pending = torch.empty(N, dtype=torch.int32, device=dev)
    entry, total = "camo_split_instances_geodesic", 0
    while True:
        call(entry, dev, *args, _stream_ptr(dev), step, _ptr(pending))
        total += step
        if not any(pending.tolist()):                              # (the host synchronisation)
            return {"labels": out, "table": table, "counts": counts, "rounds": total}
        entry, step = "camo_split_geodesic_resume", min(2 * step, _lib.SPLIT_GEO_MAX_ROUNDS)


@torch.no_grad()
def merge_parts(labels, parts, pred=None, merge=MERGE, max_instances=64):
    """``camo_split_merge``: ``labels`` as ``split_instances`` takes them and ``parts`` int32 of the same shape, its "labels" (or any
    map with a part id in 1 .. 1024 on every foreground pixel); ``pred`` as there, for the table's Sq -> {"labels": int32 [N, H, W],
    the new ids 1 .. K'' of the groups in the order of each group's smallest part id; "table": int64 [N, max_instances, 8]; "counts":
    int32 [N, 4] = (K'', part ids present, groups of two parts or more, input ids that had two parts or more and are one again;
    (-1, 0, 0, 0) for an image with a part value out of range, whose labels are then ``parts`` on the foreground)}, all on the device,
    no host synchronisation.  A part is joined to the higher part (larger peak of the squared distance to the background, equal peaks
    to the smaller part id) behind its best contact when that contact's value is at least (num / den)^2 of its own peak, ``merge`` =
    (num, den); (1, 1) joins only across a pass as high as the peak itself."""
    labels, pred = _maps(labels, pred)
    parts = label_map(parts, "parts")
    N, H, W = labels.shape
    if tuple(parts.shape) != (N, H, W):
        raise ValueError(f"need parts of labels' shape {(N, H, W)}, got {tuple(parts.shape)}")
    num, den = check_merge(merge)
    if not _integer(max_instances) or max_instances < 1:
        raise ValueError(f"max_instances must be an integer >= 1, got {max_instances!r}")
    if N * max_instances > _lib.INST_MAX_ROWS:
        raise ValueError(f"max_instances = {max_instances} for {N} images exceeds {_lib.INST_MAX_ROWS} table rows")
    labels, pred, stride = _planes(labels, pred)
    _lib.require_device(parts, "parts")
    parts = parts.detach().contiguous()
    dev = labels.device
    ws, nbytes = workspace("camo_split_merge_workspace_bytes", N, H, W, device=dev,
                           refuse=lambda: ValueError(f"camo_split_merge does not support N = {N}, H = {H}, W = {W} (a side is at most {_lib.SEG_WF_MAX_SIDE})"))
    out = torch.empty_like(labels)
    table = torch.empty(N, int(max_instances), _lib.INST_FIELDS, dtype=torch.int64, device=dev)
    counts = torch.empty(N, _lib.SPLIT_MERGE_COUNTS, dtype=torch.int32, device=dev)
    call("camo_split_merge", dev, _ptr(labels), _ptr(parts), None if pred is None else _ptr(pred), stride, N, H, W, num, den, int(max_instances),
         _ptr(out), _ptr(table), _ptr(counts), _ptr(ws), nbytes, _stream_ptr(dev))
    return {"labels": out, "table": table, "counts": counts}


def _rows(t, width, what):
    """Rows of ``width`` integers from a tensor or nested lists."""
    rows = [list(c) for c in (t.tolist() if isinstance(t, torch.Tensor) else t)]
    if any(len(c) != width for c in rows):
        raise ValueError(f"need {what} rows of {width} integers")
    return rows


def split_records(table, counts, H, W, merge_counts=None):
    """``instance_records`` on ``split_instances``' table plus its counts (tensors or nested lists; device tensors cost the one host
    copy).  Per image {"instances": [{"id", "area", "box", "centroid", "score"} in id order], "count": K', "truncated": K' > the rows
    the table holds, "split": the ids split, "cores_dropped", "left_whole": the qualifying ids past ``max_split``}.  With
    ``merge_counts`` (``split_instances(..., merge=)``'s "merge_counts"; one host copy more when it is a device tensor) the table is
    the merged one: "count" is K'', "truncated" is held to it, and every record also has "parts" (the part ids before the merge),
    "merged_groups" (the groups of two parts or more) and "made_whole" (the ids that had two parts or more and are one again)."""
    merged = None if merge_counts is None else _rows(merge_counts, _lib.SPLIT_MERGE_COUNTS, "merge_counts")
    if isinstance(table, torch.Tensor) and isinstance(counts, torch.Tensor):
        rows = table.shape[1] if table.dim() == 3 else 0
        flat = torch.cat([table.reshape(-1), counts.to(device=table.device, dtype=torch.int64).reshape(-1)]).tolist()      # (the one copy)
        nt, F, C = table.numel(), _lib.INST_FIELDS, _lib.SPLIT_COUNTS
        counts = [flat[nt + C * i: nt + C * (i + 1)] for i in range(counts.shape[0])]
        table = [[flat[(i * rows + k) * F: (i * rows + k + 1) * F] for k in range(rows)] for i in range(table.shape[0])]
    counts = [list(c) for c in counts]
    if any(len(c) != _lib.SPLIT_COUNTS for c in counts):
        raise ValueError(f"need counts rows of {_lib.SPLIT_COUNTS} integers")
    if merged is not None and len(merged) != len(counts):
        raise ValueError(f"merge_counts holds {len(merged)} images, counts {len(counts)}")
    held = counts if merged is None else merged                    # (whose first entry is the number of ids the table describes)
    base = instance_records(table, [[max(int(c[0]), 0), 0, 0, 0] for c in held], H, W)
    rec = [{"instances": r["instances"], "count": r["count"], "truncated": r["truncated"], "split": int(c[1]), "cores_dropped": int(c[2]),
            "left_whole": int(c[3])} for r, c in zip(base, counts)]
    for r, m in zip(rec, merged or ()):
        r.update({"parts": int(m[1]), "merged_groups": int(m[2]), "made_whole": int(m[3])})
    return rec


def split_options(split, instances=True):
    """The pipeline's ``split`` keyword -- ``None`` or ``False`` (off), ``True`` or a dict with any of "ratio" ((7, 10)), "min_core"
    (0), "max_split" (4), "max_instances" (64), "growth" ("euclidean"; "geodesic": connected parts), "rounds" (``None``;
    ``split_instances``') and "merge" (``None``, or a pair (num, den): ``merge_parts`` after the split) -- as a dict with the first
    four, and "growth", "rounds" and "merge" where the caller gave them (a "merge" of ``None`` is dropped), or ``None``; the
    ``ValueError`` of a bad one by name, before anything touches the device.  ``instances``: the pipeline's keyword -- the
    instances are what it splits."""
    if split is None or split is False:
        return None
    if split is True:
        split = {}
    if not isinstance(split, dict) or set(split) - set(OPTIONS) - {"growth", "rounds", "merge"}:
        raise ValueError('split must be None, False, True or a dict with any of "ratio", "min_core", "max_split", "max_instances", "growth", "rounds", '
                         f'"merge", got {split!r}')
    if not instances:
        raise ValueError("split needs instances=True: the instances are what it splits")
    opts = {**OPTIONS, **split}
    opts["ratio"] = check_arguments(**{k: opts[k] for k in OPTIONS})
    check_growth(opts.get("growth", "euclidean"), opts.get("rounds"))
    if opts.get("merge") is None:
        opts.pop("merge", None)
    else:
        opts["merge"] = check_merge(opts["merge"])
    return opts


@torch.no_grad()
def split_detected(labels, pred, opts):
    """``split_instances`` and ``split_records`` together, for the pipeline: ``split_instances``' dict plus "instances"
    (``split_records``' list).  ``opts``: ``split_options``' dict.  When an image holds more than "max_instances" parts the call is
    made once more with the table sized to the largest count, so no list is truncated.  With "merge" in ``opts`` the labels, the
    table and the records are the merged ones, the dict also holds "merge_counts", and the count that sizes the table is K''."""
    args = (opts["ratio"], opts["min_core"], opts["max_split"])
    more = {k: opts[k] for k in ("growth", "rounds", "merge") if k in opts}
    out = split_instances(labels, pred, *args, opts["max_instances"], **more)
    H, W = out["labels"].shape[1:]
    rec = split_records(out["table"], out["counts"], H, W, out.get("merge_counts"))
    if any(r["truncated"] for r in rec):
        out = split_instances(labels, pred, *args, max(r["count"] for r in rec), **more)
        rec = split_records(out["table"], out["counts"], H, W, out.get("merge_counts"))
    out["instances"] = rec
    return out
