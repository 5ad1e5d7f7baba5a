"""Developer aid / measurement of instance contours (include/camo_contours.h):
  python tools/dev/dev_contours_bench.py calls     microseconds per call of camo_contours at N = 16 of 256 x 256 at the default capacity
                                                   (min(4 H W, CAMO_CONTOUR_LDS_CRACKS) cracks: the LDS form) and at one 1024 x 1024 with
                                                   the capacity the next power of two above its cracks and above the LDS form's (the
                                                   global form), on the label maps camo_instances makes of dev_instances_bench.py's
                                                   blob-like mask (connectivity 8); beside each time camo_rle_runs' on the same maps, the
                                                   launch count, and the wall time of encode_instance_polygons and of encode_instances,
                                                   host work and copies included
  python tools/dev/dev_contours_bench.py loop 16   one batch size only, 200 calls (50 at 1024 x 1024) of camo_contours (for a kernel trace)
The library is called directly with every buffer allocated beforehand; every case is warmed up; a window is 200 calls between two
device events (50 at 1024 x 1024), the smallest of five windows is the figure and the largest is printed beside it; a wall time is
the smallest of three calls after a warm-up.  The outputs of every timed case are checked against the restatement
(tests/contours_ref.py).  No time is asserted."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contours_ref as R
from dev_instances_bench import SIZES, inputs
from dev_rle_bench import wall
from dev_timing import timed

RUNS = 1 << 17                      # camo_rle_runs' capacity: holds every run of both sizes


def label_maps(N, H, W):
    import torch
    from camouflage_multimodal_amd import mask_instances
    return mask_instances(torch.from_numpy(inputs(N, H, W)["blobs"]).cuda(), 0.5, 8, 0, False, 64)["labels"]


def capacity(labels):
    """(C, launches): 256 x 256 at the default capacity, 1024 x 1024 from twice the LDS form's; doubled until it holds every image's cracks."""
    from camouflage_multimodal_amd import _lib, contours
    N, H, W = labels.shape
    C = min(4 * H * W, _lib.CONTOUR_LDS_CRACKS) * (1 if H * W <= 256 * 256 else 2)
    most = int(contours.trace_contours(labels)["counts"][:, 0].max())
    while C < most:
        C *= 2
    C = min(C, 4 * H * W)
    return C, 6 if C <= _lib.CONTOUR_LDS_CRACKS else 5 + 2 * (C - 1).bit_length()


def prepared(labels, C):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd._lib import _ptr, _stream_ptr
    L, dev, (N, H, W) = _lib.lib(), labels.device, labels.shape
    Rr, V, st = max(1, C // 4), C, _stream_ptr(labels.device)
    nbytes = L.camo_contours_workspace_bytes(N, H, W, C, Rr, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rings, xy = torch.empty(N, Rr, 5, dtype=torch.int64, device=dev), torch.empty(N, V, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(N, 6, dtype=torch.int32, device=dev)
    rbytes = L.camo_rle_runs_workspace_bytes(N, H, W, RUNS)
    rws = torch.empty(rbytes, dtype=torch.uint8, device=dev)
    runs, rcounts = torch.empty(N, RUNS, 2, dtype=torch.int32, device=dev), torch.empty(N, 2, dtype=torch.int32, device=dev)

    def trace():
        rc = L.camo_contours(_ptr(labels), N, H, W, 8, C, Rr, V, _ptr(rings), _ptr(xy), _ptr(counts), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())

    def rle():
        rc = L.camo_rle_runs(_ptr(labels), N, H, W, RUNS, _ptr(runs), _ptr(rcounts), _ptr(rws), rbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return trace, rle, (rings, xy, counts), rcounts, nbytes


def calls():
    from camouflage_multimodal_amd import contours, encode_instances
    for N, H, W, iters in SIZES:
        labels = label_maps(N, H, W)
        C, launches = capacity(labels)
        trace, rle, out, rcounts, nbytes = prepared(labels, C)
        t, tr = timed(trace, iters), timed(rle, iters)
        got = [a.cpu().numpy() for a in out]
        want = R.contours(labels[:1].cpu().numpy(), 8, C, max(1, C // 4), C)
        same = all(np.array_equal(g[0], w[0]) for g, w in zip(got, want))
        c = got[2]
        print(f"N = {N:2d}, {H} x {W}, C = {C} ({'LDS' if launches == 6 else 'global'} form, {launches} launches, workspace {nbytes / 2 ** 20:.1f} MiB): camo_contours "
              f"{t[0]:.1f} us (up to {t[1]:.1f}) per call; camo_rle_runs on the same maps {tr[0]:.1f} us (up to {tr[1]:.1f}), 3 launches; per image up to "
              f"{int(c[:, 0].max())} cracks, {int(c[:, 1].max())} rings, {int(c[:, 2].max())} vertices, {int(rcounts[:, 0].max())} runs, {int(labels.max())} ids; "
              f"image 0 {'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)
        tp, polys = wall(lambda: contours.encode_instance_polygons(labels))
        te, _ = wall(lambda: encode_instances(labels))
        areas = all({i: e["area"] for i, e in p.items()} == {int(i): int(n) for i, n in zip(*np.unique(l[l > 0], return_counts=True))}
                    for p, l in zip(polys, labels.cpu().numpy()))
        print(f"        encode_instance_polygons {tp:.0f} us wall; encode_instances {te:.0f} us wall; every id's area {'equal to' if areas else 'DIFFERENT FROM'} its pixel count",
              flush=True)


def loop(n):
    import torch
    for N, H, W, iters in SIZES:
        if N != int(n): continue
        labels = label_maps(N, H, W)
        trace = prepared(labels, capacity(labels)[0])[0]
        for _ in range(iters): trace()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"calls": calls, "loop": loop}[sys.argv[1]](*sys.argv[2:3])
