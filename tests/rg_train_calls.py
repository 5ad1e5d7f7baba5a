"""The region-graph training call (include/camo_rg_train.h, _bn.h, _drop.h, camo_rg_pixel_loss.h) made directly, stated once for the
four entries (a helper module, not a conftest; it imports no test module).

Each entry takes the arguments of the one before it and its own, the stream last: the 23 shared arguments, then the batch-norm tail
(momentum, running, batch_stats), then (batch_stats_mode, the three rates, seed), then (node_w, node_off, n_images, radius, w_pixel).
``direct`` makes the call on buffers between the guard bands of tests/guarded.py; ``refuse`` makes it on fake pointers, for the
argument checks, which all run on the host before any launch."""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from guarded import Arrays

ENTRIES = ("camo_rg_loss_backward", "camo_rg_loss_backward_bn", "camo_rg_loss_backward_drop", "camo_rg_loss_backward_pixel")
STAT_NAMES = tuple(f"bn{k}.running_{s}" for k in (1, 2, 3, 4) for s in ("mean", "var"))       # the order of the `running` table
RUNNING_SLOTS = (6, 7, 12, 13, 18, 19, 24, 25)       # of the 28-slot parameter table: not read under batch statistics
FAKE = 0x1000                                        # never dereferenced
# table_null -> (the table, its null slots)
HOLES = {"params": ("params", (5,)), "running slots of params": ("params", RUNNING_SLOTS), "grads": ("grads", (31,)), "running": ("running", (7,))}


def _lib():
    from camouflage_multimodal_amd import _lib as B
    return B


def _need(entry, dims, nc, N, E, mode):
    """The entry's own workspace query."""
    L, i = _lib().lib(), ENTRIES.index(entry)
    if i < 2:
        return (L.camo_rg_train_workspace_bytes, L.camo_rg_train_bn_workspace_bytes)[i](ctypes.byref(dims), nc, N, E)
    return L.camo_rg_train_drop_workspace_bytes(ctypes.byref(dims), nc, N, E, mode)


def _call(entry, common, bn, drop, pixel, stream):
    own = (bn, drop, pixel)[:ENTRIES.index(entry)]
    return getattr(_lib().lib(), entry)(*common, *(v for part in own for v in part), stream)


def direct(entry, model, x, csr_pair, targets, weights=(1.0, 1.0, 1.0), mode=0, rates=(0.0, 0.0, 0.0), seed=0, momentum=0.1, pixel=None):
    """``entry`` called as the wrapper calls it, on a workspace of exactly its ``*_workspace_bytes`` filled with 0xA5 and on outputs of
    exactly their sizes filled with 0xFF (a NaN in every float) -- the 32 gradients, the loss (4 floats, 6 for the pixel entry) and under
    batch statistics batch_stats [4, 2, C] -- and eight running-statistic buffers that start as ``model``'s, each in a guarded tensor of
    its own.  ``mode`` (1: batch statistics), ``rates`` and ``seed`` are the dropout and pixel entries'; the two older entries have their
    mode.  ``pixel`` = (node_w int64 [n, 2], node_off int32 [images + 1], radius, w_pixel), device tensors.  Asserted: the return code,
    every guard, that every output element is finite, hence written, and that ``model``, whose tables were passed, is unchanged.
    Returns a record: loss, grads (32 views in the parameters' shapes), bs and run (8 tensors in STAT_NAMES order; both None without
    batch statistics), need."""
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    assert (pixel is not None) == (entry == ENTRIES[3])
    mode = (0, 1, mode, mode)[ENTRIES.index(entry)]
    csr, rcsr = csr_pair
    x = x.contiguous()
    ins = (x, *csr, *rcsr, *targets)
    i32, f32 = torch.int32, torch.float32
    assert all(a.is_cuda and a.is_contiguous() for a in ins) and [a.dtype for a in ins] == [f32, i32, i32, f32, i32, i32, f32, i32, i32, f32]
    n, E, C, nc = x.shape[0], csr[1].shape[0], model._dims.hidden, model.num_classes
    need = _need(entry, model._dims, nc, n, E, mode)
    assert need > 0
    params = model.trainable_parameters()
    spec = {"workspace": need, **{f"grad{i}": ((p.numel(),), np.float32) for i, p in enumerate(params)},
            "loss": ((4 if pixel is None else 6,), np.float32)}
    if mode:
        spec.update({"batch_stats": ((4, 2, C), np.float32), **{k: ((C,), np.float32) for k in STAT_NAMES}})
    A = Arrays(spec, {None: 0xFF, "workspace": 0xA5})
    out = {k: A.piece[k].view(f32) for k in spec if k != "workspace"}
    assert all(bool(torch.isnan(v).all()) for v in out.values())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    if mode:
        for k in STAT_NAMES:
            out[k].copy_(before[k])
    tab, keep = model._param_table()
    htab, hkeep = model._head_table()
    gtab = (ctypes.c_void_p * len(params))(*[A.ptr(f"grad{i}") for i in range(len(params))])
    rtab = (ctypes.c_void_p * 8)(*[A.ptr(k) for k in STAT_NAMES]) if mode else None
    common = (ctypes.byref(model._dims), nc, tab, htab, *(_ptr(a) for a in ins[:7]), n, E, *(_ptr(a) for a in ins[7:]), *weights,
              A.ptr("workspace"), need, A.ptr("loss"), gtab)
    bn = (momentum, rtab, A.ptr("batch_stats")) if mode else (0.0, None, None)
    own = () if pixel is None else (_ptr(pixel[0]), _ptr(pixel[1]), pixel[1].numel() - 1, pixel[2], pixel[3])
    _lib().check(_call(entry, common, bn, (mode, *rates, seed), own, _stream_ptr()), entry)
    A.check_guards()                                                     # (synchronises first)
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), f"{k}: an element was not written"
    for k, v in model.state_dict().items():                             # `running` was written, not the model
        assert torch.equal(v, before[k]), k
    return SimpleNamespace(loss=out["loss"], grads=[out[f"grad{i}"].view(p.shape) for i, p in enumerate(params)],
                           bs=out["batch_stats"].view(4, 2, C) if mode else None, run=[out[k] for k in STAT_NAMES] if mode else None, need=need)


def refuse(entry, hidden=128, heads=4, nc=2, N=23, E=100, ws_bytes=None, null=(), table_null=None, momentum=0.1, running=False, stats=False,
           mode=0, rates=(0.0, 0.0, 0.0), seed=0, n_images=1, radius=15, w_pixel=1.0):
    """``entry`` on fake pointers, for a call the library has to refuse: SOMETHING in it must be wrong, or kernels are launched on the
    fakes.  ``ws_bytes`` None: what the entry's workspace query says.  ``null``: one name or several among x, rowptr, col, w, rrowptr,
    rcol, rw, mt, it, et, ws, loss, params, heads, grads, node_w, node_off.  ``table_null``: a key of HOLES.  ``running`` / ``stats``:
    whether the table of eight and batch_stats are given.  Returns (return code, the library's message, the workspace query)."""
    L = _lib().lib()
    d = _lib().CamoRgDims(15, hidden, heads)
    need = _need(entry, d, nc, N, E, mode)
    null = (null,) if isinstance(null, str) else tuple(null)
    holed, holes = HOLES[table_null] if table_null is not None else (None, ())

    def tab(name, n):
        return None if name in null else (ctypes.c_void_p * n)(*[None if name == holed and i in holes else FAKE for i in range(n)])

    def p(*names):
        return tuple(None if k in null else FAKE for k in names)

    common = (ctypes.byref(d), nc, tab("params", 28), tab("heads", 12), *p("x", "rowptr", "col", "w", "rrowptr", "rcol", "rw"), N, E,
              *p("mt", "it", "et"), 1.0, 1.0, 1.0, *p("ws"), need if ws_bytes is None else ws_bytes, *p("loss"), tab("grads", 32))
    bn = (momentum, tab("running", 8) if running else None, FAKE if stats else None)
    rc = _call(entry, common, bn, (mode, *rates, seed), (*p("node_w", "node_off"), n_images, radius, w_pixel), None)
    return rc, L.camo_last_error(), need
