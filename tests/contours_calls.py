"""camo_contours (include/camo_contours.h) as a tests/raw_calls.py Call, stated once (a helper module, not a conftest):
tests/test_contours.py runs it between guards on memory the call did not clear."""
import numpy as np
import torch

from raw_calls import Call, execute

NAMES = ("rings", "xy", "counts")


def contours_call(labels, connectivity, C, R, V):
    from camouflage_multimodal_amd import _lib
    L, (N, H, W) = _lib.lib(), labels.shape
    nbytes = L.camo_contours_workspace_bytes(N, H, W, C, R, V)
    assert nbytes > 0 and nbytes % 256 == 0
    outs = {"rings": ((N, R, 5), np.int64), "xy": ((N, V, 2), np.int32), "counts": ((N, 6), np.int32)}
    return Call(outs, nbytes, lambda p, w, nb: L.camo_contours(p["labels"], N, H, W, connectivity, C, R, V, p["rings"], p["xy"], p["counts"], w, nb,
                                                               torch.cuda.current_stream().cuda_stream), {"labels": np.asarray(labels, np.int32)})


def run(labels, connectivity, C, R, V, fill=0xA5, ws_fill=0xFF, before=()):
    return execute(contours_call(labels, connectivity, C, R, V), fill, before=before, ws_fill=ws_fill, skew=8)
