"""Every raw ctypes call of the image and region-graph pipeline, and the grouped GEMM's two testing hooks, stated once, on the one guard
harness (a helper module, not a conftest).

``BUILDERS`` maps an entry point's name to a function from data -- numpy arrays and parameters, never a test's name -- to a ``Call``;
``execute`` runs a Call with every caller array in a guarded piece of tests/guarded.py: the inputs copied in before each call and held
unchanged after the last, the outputs and the workspace of exactly ``*_workspace_bytes`` filled with the byte the test names.  The
modules' tests choose the cases, the fills and the skew; tests/test_caller_memory.py runs the same calls on dirty memory; and
tests/test_guarded.py holds the harness itself, with a fake call on CPU tensors, and this table to the headers' symbols."""
import ctypes
import math

import numpy as np
import torch

from guarded import Arrays


def _lib():
    from camouflage_multimodal_amd import _lib as B
    return B.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sized(nbytes):
    assert nbytes > 0 and nbytes % 256 == 0, nbytes
    return nbytes


def _bytes(a):
    return torch.from_numpy(np.array(a, order="C").reshape(-1).view(np.uint8))      # (a writable copy: cached cases are read-only)


def fractions(thr):
    """Fractions -> (their numerators over the common denominator, that denominator)."""
    den = 1
    for f in thr:
        den = den * f.denominator // math.gcd(den, f.denominator)
    return [int(f * den) for f in thr], int(den)


def same_bytes(got, want, what, names=None):
    """The arrays ``names`` of two dicts (default: all, and the same ones in both) have one dtype, one shape and the same bytes."""
    if names is None:
        assert sorted(got) == sorted(want)
    for k in want if names is None else names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, np.argwhere(g != w)[:5].tolist())


class Call:
    """One call of an entry point: ``outs`` name -> (shape, dtype) of the caller arrays it writes, ``ws`` its workspace size in bytes
    (0: it takes none), ``invoke(ptr, ws_ptr, ws_bytes)`` -> the return code, ``ins`` name -> the array an input holds (a zero-size
    input is passed as a null pointer), ``init`` name -> the array an in-out argument holds on entry."""

    def __init__(self, outs, ws, invoke, ins=None, init=None):
        self.outs, self.ws, self.invoke = outs, int(ws), invoke
        self.ins, self.init = ({k: np.asarray(a) for k, a in (d or {}).items()} for d in (ins, init))
        assert not set(self.outs) & set(self.ins) and "ws" not in set(self.outs) | set(self.ins)


def execute(call, fill, before=(), ws_fill=None, skew=0, device="cuda", error_text=None):
    """``call`` on outputs filled with ``fill`` that begin ``skew`` bytes past a 256-byte boundary and a workspace filled with ``ws_fill``
    (default: ``fill``), after the calls of ``before`` on the same buffers -> the outputs as numpy.  Asserted: every return code
    (``error_text()`` is the message), every guard after every call, the workspace past the size ``call`` was given, and the inputs'
    bytes after the last call."""
    calls = list(before) + [call]
    spec = dict(call.outs)
    for c in calls:
        for k, a in c.ins.items():
            spec[k] = max(spec.get(k, 0), a.nbytes)
    if call.ws:
        spec["ws"] = max(c.ws for c in calls)
    A = Arrays(spec, {None: fill, "ws": fill if ws_fill is None else ws_fill}, {None: 0, **dict.fromkeys(call.outs, skew)}, device)
    for c in calls:
        for k, (shape, dtype) in c.outs.items():
            assert int(np.prod(shape)) * np.dtype(dtype).itemsize == A.nbytes(k), (k, shape)
        if c is call and call.ws:
            A.refill("ws", call.ws)
        for k, a in {**c.ins, **c.init}.items():
            A.piece[k][:a.nbytes].copy_(_bytes(a))
        ptr = {k: A.ptr(k) for k in c.outs}
        ptr.update({k: A.ptr(k) if a.nbytes else None for k, a in c.ins.items()})
        rc = c.invoke(ptr, A.ptr("ws") if c.ws else None, c.ws)
        assert rc == 0, (error_text or _lib().camo_last_error)()
        A.check_guards()
    got = A.collect()
    if call.ws:
        assert A.tail_intact("ws", call.ws), "the workspace was written past the size the call was given"
    for k, a in call.ins.items():
        assert got[k][:a.nbytes].tobytes() == _bytes(a).numpy().tobytes(), f"the input {k} was written"
    return {k: got[k] for k in call.outs}


# ---- one builder per entry point ------------------------------------------------------------------------------------------

def canny(img, sigma, low, high):
    L, (N, H, W) = _lib(), img.shape[:3]
    return Call({"edges": ((N, H, W), np.uint8), "grad": ((N, 3, H, W), np.float32)}, _sized(L.camo_canny_workspace_bytes(N, H, W)),
                lambda p, w, nb: L.camo_canny(p["image"], N, H, W, sigma, low, high, w, nb, p["edges"], p["grad"], _stream()), {"image": img})


def canny_hysteresis(cls):
    L, (N, H, W) = _lib(), cls.shape
    return Call({"edges": ((N, H, W), np.uint8)}, _sized(L.camo_canny_workspace_bytes(N, H, W)),
                lambda p, w, nb: L.camo_canny_hysteresis(p["classes"], N, H, W, w, nb, p["edges"], _stream()), {"classes": np.asarray(cls, np.uint8)})


def slic(img, n, compactness, sigma):
    L, (N, H, W) = _lib(), img.shape[:3]
    return Call({"labels": ((N, H, W), np.int32), "counts": ((N, 2), np.int32)}, _sized(L.camo_slic_workspace_bytes(N, H, W, n)),
                lambda p, w, nb: L.camo_slic(p["image"], N, H, W, n, compactness, sigma, w, nb, p["labels"], p["counts"], _stream()), {"image": img})


def slic_connect(maps, min_size, max_size):
    L, (N, H, W) = _lib(), maps.shape
    return Call({"labels": ((N, H, W), np.int32), "counts": ((N, 2), np.int32)}, _sized(L.camo_slic_workspace_bytes(N, H, W, 0)),
                lambda p, w, nb: L.camo_slic_connect(p["maps"], N, H, W, min_size, max_size, w, nb, p["labels"], p["counts"], _stream()),
                {"maps": np.asarray(maps, np.int32)})


def slic_update(lab, near, cent):
    """``sums`` is scratch (any content on entry, nothing promised on exit); ``centroids`` is in-out and holds ``cent`` on entry."""
    L, (N, H, W), K = _lib(), near.shape, cent.shape[1]
    return Call({"sums": ((N, K, 6), np.int64), "centroids": ((N, K, 5), np.float32)}, 0,
                lambda p, w, nb: L.camo_slic_update(p["lab"], p["near"], N, H, W, K, p["sums"], p["centroids"], _stream()),
                {"lab": np.asarray(lab, np.float32), "near": np.asarray(near, np.int32)}, init={"centroids": np.asarray(cent, np.float32)})


def rg_region_graph(img, seg, canny_map, n_labels, cap):
    L, (H, W) = _lib(), seg.shape
    outs = {"x": ((n_labels, 15), np.float32), "region_map": ((n_labels,), np.int32), "edge_index": ((2, cap), np.int64),
            "edge_attr": ((cap,), np.float32), "counts": ((2,), np.int32)}
    return Call(outs, _sized(L.camo_rg_graph_workspace_bytes(n_labels)),
                lambda p, w, nb: L.camo_rg_region_graph(p["image"], p["segments"], p["canny"], H, W, n_labels, w, nb, p["x"], p["region_map"],
                                                        p["edge_index"], p["edge_attr"], cap, p["counts"], _stream()),
                {"image": img, "segments": seg, "canny": canny_map})


def rg_region_graph_batch(img, seg, canny_map, lb, cap):
    L, (N, H, W) = _lib(), seg.shape
    nodes = N * lb
    outs = {"x": ((nodes, 15), np.float32), "region_map": ((N, lb), np.int32), "edge_index": ((2, cap), np.int64), "edge_attr": ((cap,), np.float32),
            "node_off": ((N + 1,), np.int32), "edge_off": ((N + 1,), np.int32), "batch": ((nodes,), np.int32), "status": ((2,), np.int32)}
    return Call(outs, _sized(L.camo_rg_batch_workspace_bytes(N, H, W, lb)), lambda p, w, nb: L.camo_rg_region_graph_batch(
        p["image"], p["segments"], p["canny"], N, H, W, lb, w, nb, p["x"], nodes, p["region_map"], p["edge_index"], p["edge_attr"], cap,
        p["node_off"], p["edge_off"], p["batch"], p["status"], _stream()), {"image": img, "segments": seg, "canny": canny_map})


def rg_node_targets(seg, rmap, off, gt, inst, edge, n_nodes, band, emin):
    """``inst`` and ``edge`` may be None: the optional masks, passed as null pointers."""
    L, (N, H, W) = _lib(), seg.shape
    names = ("segments", "region_map", "node_off", "gt", "inst", "edge")
    ins = {k: a for k, a in zip(names, (seg, rmap, np.asarray(off, np.int32), gt, inst, edge)) if a is not None}
    outs = {"counts": ((n_nodes, 4), np.int32), "mask_t": ((n_nodes,), np.int32), "inst_t": ((n_nodes,), np.int32), "edge_t": ((n_nodes,), np.float32)}
    return Call(outs, 0, lambda p, w, nb: L.camo_rg_node_targets(*(p.get(k) for k in names), N, H, W, rmap.shape[1], n_nodes, band, emin,
                                                                 p["counts"], p["mask_t"], p["inst_t"], p["edge_t"], _stream()), ins)


def instances(pred, threshold, connectivity, min_area, fill_holes, rows):
    L, (N, H, W) = _lib(), pred.shape
    outs = {"labels": ((N, H, W), np.int32), "clean": ((N, H, W), np.uint8), "table": ((N, rows, 8), np.int64), "counts": ((N, 4), np.int32)}
    return Call(outs, _sized(L.camo_instances_workspace_bytes(N, H, W)),
                lambda p, w, nb: L.camo_instances(p["pred"], H * W, threshold, N, H, W, connectivity, min_area, int(fill_holes), rows,
                                                  p["labels"], p["clean"], p["table"], p["counts"], w, nb, _stream()), {"pred": pred})


MATCH_NAMES = ("inter", "pred_rows", "gt_area", "match", "gt_match", "counts")
BOUNDARY_MATCH_NAMES = ("inter", "inter_bd", "pred_rows", "gt_area", "match", "gt_match", "counts")


def inst_match(pred, gt, P, G, table, thr):
    L, (N, H, W), T = _lib(), pred.shape, len(thr)
    nums, den = fractions(thr)
    shapes = {"inter": (N, P + 1, G + 1), "pred_rows": (N, P, 4), "gt_area": (N, G), "match": (N, T, P), "gt_match": (N, T, G), "counts": (N, 4)}
    ins = {"pred": pred, "gt": gt, **({} if table is None else {"table": table})}
    return Call({k: (shapes[k], np.int32) for k in MATCH_NAMES}, _sized(L.camo_inst_match_workspace_bytes(N, H, W, P, G, T)),
                lambda p, w, nb: L.camo_inst_match(p["pred"], p["gt"], N, H, W, P, G, None if table is None else p["table"],
                                                   0 if table is None else table.shape[1], (ctypes.c_int32 * T)(*nums), den, T,
                                                   *(p[k] for k in MATCH_NAMES), w, nb, _stream()), ins)


def rle_runs(labels, R):
    L, (N, H, W) = _lib(), labels.shape
    return Call({"runs": ((N, R, 2), np.int32), "counts": ((N, 2), np.int32)}, _sized(L.camo_rle_runs_workspace_bytes(N, H, W, R)),
                lambda p, w, nb: L.camo_rle_runs(p["labels"], N, H, W, R, p["runs"], p["counts"], w, nb, _stream()), {"labels": labels})


def rle_decode(arrays, N, H, W):
    """``arrays``: (cnts, ann_off, ann_image, ann_value) as tests/rle_ref.py takes them."""
    L = _lib()
    ins = {k: np.asarray(v, np.int32).reshape(-1) for k, v in zip(("cnts", "ann_off", "ann_image", "ann_value"), arrays)}
    A, total = len(ins["ann_image"]), len(ins["cnts"])
    return Call({"labels": ((N, H, W), np.int32), "ann_sum": ((A,), np.int64)}, _sized(L.camo_rle_decode_workspace_bytes(N, H, W, A, total)),
                lambda p, w, nb: L.camo_rle_decode(p["cnts"], total, p["ann_off"], p["ann_image"], p["ann_value"], A, N, H, W, p["labels"], p["ann_sum"],
                                                   w, nb, _stream()), ins)


def guided_filter(guide, p_map, C, r, eps):
    L, (N, H, W) = _lib(), p_map.shape
    return Call({"q": ((N, H, W), np.float32), "coef": ((N, C + 1, H, W), np.float32)}, _sized(L.camo_guided_workspace_bytes(N, H, W, C)),
                lambda q, w, nb: L.camo_guided_filter(q["guide"], q["p"], H * W, N, H, W, C, r, eps, 0, q["q"], q["coef"], w, nb, _stream()),
                {"guide": guide, "p": p_map})


def _channel(maps, channel, gt):
    """(offset in bytes of ``channel`` in the first image of maps fp32 [N, C, H, W], which is read in place; an image's stride in elements)"""
    assert maps.dtype == np.float32 and maps.shape[0] == gt.shape[0] and maps.shape[2:] == gt.shape[1:]
    return 4 * channel * gt.shape[1] * gt.shape[2], maps.shape[1] * gt.shape[1] * gt.shape[2]


def seg_histograms(maps, channel, gt):
    L, (N, H, W), (at, stride) = _lib(), gt.shape, _channel(maps, channel, gt)
    return Call({"hist": ((N, 4, 2, 256), np.int32), "split": ((N, 2), np.int32)}, 0,
                lambda p, w, nb: L.camo_seg_histograms(p["maps"] + at, stride, p["gt"], N, H, W, p["hist"], p["split"], _stream()), {"maps": maps, "gt": gt})


def seg_weighted_f(maps, channel, gt):
    from camouflage_multimodal_amd.seg_measures import gaussian_7x7
    L, (N, H, W), (at, stride) = _lib(), gt.shape, _channel(maps, channel, gt)
    return Call({"sums": ((N, 3), np.int64)}, _sized(L.camo_seg_weighted_f_workspace_bytes(N, H, W)),
                lambda p, w, nb: L.camo_seg_weighted_f(p["maps"] + at, stride, p["gt"], N, H, W, p["gauss"], w, nb, p["sums"], _stream()),
                {"maps": maps, "gt": gt, "gauss": np.asarray(gaussian_7x7(), np.float64).reshape(-1)})


def seg_counts(maps, channel, gt, threshold):
    L, (N, H, W), (at, stride) = _lib(), gt.shape, _channel(maps, channel, gt)
    return Call({"counts": ((N, 5), np.int64)}, 0,
                lambda p, w, nb: L.camo_seg_counts(p["maps"] + at, stride, p["gt"], threshold, N, H, W, p["counts"], _stream()), {"maps": maps, "gt": gt})


def boundary_labels(lab, d):
    L, (N, H, W) = _lib(), lab.shape
    return Call({"out": ((N, H, W), np.int32)}, _sized(L.camo_boundary_labels_workspace_bytes(N, H, W, d)),
                lambda p, w, nb: L.camo_boundary_labels(p["labels"], N, H, W, d, p["out"], w, nb, _stream()), {"labels": lab})


def boundary_match(pred, gt, pb, gb, P, G, table, thr):
    L, (N, H, W), T = _lib(), pred.shape, len(thr)
    nums, den = fractions(thr)
    shapes = {"inter": (N, P + 1, G + 1), "inter_bd": (N, P + 1, G + 1), "pred_rows": (N, P, 6), "gt_area": (N, G, 2), "match": (N, T, P),
              "gt_match": (N, T, G), "counts": (N, 4)}
    ins = {"pl": pred, "gl": gt, "pb": pb, "gb": gb, **({} if table is None else {"table": table})}
    return Call({k: (shapes[k], np.int32) for k in BOUNDARY_MATCH_NAMES}, _sized(L.camo_boundary_match_workspace_bytes(N, H, W, P, G, T)),
                lambda p, w, nb: L.camo_boundary_match(p["pl"], p["gl"], p["pb"], p["gb"], N, H, W, P, G, None if table is None else p["table"],
                                                       0 if table is None else table.shape[1], (ctypes.c_int32 * T)(*nums), den, T,
                                                       *(p[k] for k in BOUNDARY_MATCH_NAMES), w, nb, _stream()), ins)


def poly_decode(arrays, N, H, W):
    """``arrays``: (xy, poly_off, ann_poly_off, ann_image, ann_value) as tests/poly_ref.py gives them."""
    L = _lib()
    xy, poly_off, ann_poly_off, img, val = arrays
    ins = {"xy": np.ascontiguousarray(xy, np.float64).reshape(-1), "poly_off": np.asarray(poly_off, np.int32), "ann_poly_off": np.asarray(ann_poly_off, np.int32),
           "ann_image": np.asarray(img, np.int32), "ann_value": np.asarray(val, np.int32)}
    A, Pn, V = len(img), len(poly_off) - 1, len(xy)
    return Call({"labels": ((N, H, W), np.int32), "ann_area": ((A,), np.int64)}, _sized(L.camo_poly_decode_workspace_bytes(N, H, W, A, Pn, V)),
                lambda p, w, nb: L.camo_poly_decode(p["xy"], V, p["poly_off"], Pn, p["ann_poly_off"], p["ann_image"], p["ann_value"], A, N, H, W,
                                                    p["labels"], p["ann_area"], w, nb, _stream()), ins)


# ---- the grouped GEMM's testing hooks (include/camo_fusion.h; not pipeline calls, so not in BUILDERS) --------------------------------------
# A problem is a dict: M, N, K, lda, ldb, ldc, flags and, where they are not the defaults, ldr, drop_site, uniform_n, aux_scale; A, B, C
# and, where present, bias, res, bias_grad, row_sample, inv_nr = (name of a caller array, offset into it in 4-byte elements).  An operand
# that must start off a 16-byte boundary has offset 1: every array begins on a 256-byte boundary (execute's skew stays 0).  ``ins`` name
# -> the array an input holds, ``outs`` name -> (shape, dtype) of the arrays the launch writes (several problems may name one), ``init``
# name -> what an accumulator (C with GF_ATOMIC, bias_grad) holds on entry.  ``rc``: a list that takes the return code of a launch that
# is expected to be refused (the Call then reports success, and the caller asserts the code and the untouched fill).
GEMM_POINTERS = ("A", "B", "C", "bias", "res", "bias_grad", "row_sample", "inv_nr")
GEMM_INTS = ("M", "N", "K", "lda", "ldb", "ldc", "ldr", "flags", "drop_site", "uniform_n")


def _gemm_address(p, prob, k):
    return None if prob.get(k) is None else p[prob[k][0]] + 4 * prob[k][1]


def _gemm_rc(code, rc):
    if rc is None:
        return code
    rc.append(code)
    return 0


def gemm(prob, prec, ins, outs, init=None, rc=None):
    """One problem through camo_debug_gemm (which has no aux_scale, sample map, dropout: those go through gemm_batch)."""
    L = _lib()
    assert prob.get("aux_scale", 1.0) == 1.0 and not any(prob.get(k) for k in ("row_sample", "inv_nr", "uniform_n", "drop_site"))
    a = lambda p, k: _gemm_address(p, prob, k)
    return Call(outs, 0, lambda p, w, nb: _gemm_rc(L.camo_debug_gemm(
        a(p, "A"), prob["lda"], a(p, "B"), prob["ldb"], a(p, "C"), prob["ldc"], a(p, "bias"), a(p, "res"), prob.get("ldr", 0), a(p, "bias_grad"),
        prob["M"], prob["N"], prob["K"], prob["flags"], prec, _stream()), rc), ins, init)


def gemm_batch(probs, prec, ins, outs, init=None, drop_p=0.0, seed=0, rc=None):
    """``probs`` in ONE launch through camo_debug_gemm_batch."""
    L, n = _lib(), len(probs)

    def invoke(p, w, nb):
        ptrs = (ctypes.c_void_p * (8 * n))(*(_gemm_address(p, q, k) for q in probs for k in GEMM_POINTERS))
        ints = (ctypes.c_int32 * (10 * n))(*(int(q.get(k, 0)) for q in probs for k in GEMM_INTS))
        aux = (ctypes.c_float * n)(*(float(q.get("aux_scale", 1.0)) for q in probs))
        return _gemm_rc(L.camo_debug_gemm_batch(ptrs, ints, aux, n, prec, drop_p, seed, _stream()), rc)
    return Call(outs, 0, invoke, ins, init)


BUILDERS = {
    "camo_canny": canny, "camo_canny_hysteresis": canny_hysteresis, "camo_slic": slic, "camo_slic_connect": slic_connect, "camo_slic_update": slic_update,
    "camo_rg_region_graph": rg_region_graph, "camo_rg_region_graph_batch": rg_region_graph_batch, "camo_rg_node_targets": rg_node_targets,
    "camo_instances": instances, "camo_inst_match": inst_match, "camo_rle_runs": rle_runs, "camo_rle_decode": rle_decode,
    "camo_guided_filter": guided_filter, "camo_seg_histograms": seg_histograms, "camo_seg_weighted_f": seg_weighted_f, "camo_seg_counts": seg_counts,
    "camo_boundary_labels": boundary_labels, "camo_boundary_match": boundary_match, "camo_poly_decode": poly_decode,
}
