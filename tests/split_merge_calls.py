"""camo_split_merge (include/camo_split_merge.h) as a tests/raw_calls.py Call, stated once (a helper module, not a conftest):
tests/test_split_merge.py runs it between guards on memory the call did not clear."""
import numpy as np
import torch

from raw_calls import Call, execute

NAMES = ("labels", "table", "counts")


def merge_call(lab, parts, pred=None, channel=0, merge=(4, 5), rows=64):
    """``pred``: None, fp32 [N, H, W], or fp32 [N, C, H, W] whose ``channel`` is read in place."""
    from camouflage_multimodal_amd import _lib
    L, (N, H, W) = _lib.lib(), lab.shape
    assert parts.shape == lab.shape
    at, stride, ins = 0, 0, {"labels": np.asarray(lab, np.int32), "parts": np.asarray(parts, np.int32)}
    if pred is not None:
        ins["pred"] = pred = np.asarray(pred, np.float32)
        at, stride = (4 * channel * H * W, pred.shape[1] * H * W) if pred.ndim == 4 else (0, H * W)
    nbytes = L.camo_split_merge_workspace_bytes(N, H, W)
    assert nbytes > 0 and nbytes % 256 == 0
    outs = {"labels_out": ((N, H, W), np.int32), "table": ((N, rows, 8), np.int64), "counts": ((N, 4), np.int32)}
    return Call(outs, nbytes, lambda p, w, nb: L.camo_split_merge(p["labels"], p["parts"], p["pred"] + at if pred is not None else None, stride, N, H, W,
                                                                  merge[0], merge[1], rows, p["labels_out"], p["table"], p["counts"], w, nb,
                                                                  torch.cuda.current_stream().cuda_stream), ins)


def run(lab, parts, pred=None, channel=0, fill=0xA5, ws_fill=0xFF, before=(), **p):
    got = execute(merge_call(lab, parts, pred, channel, **p), fill, before=before, ws_fill=ws_fill, skew=8)
    return {"labels": got["labels_out"], "table": got["table"], "counts": got["counts"]}
