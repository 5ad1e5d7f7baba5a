"""Developer aid / measurement of the benchmark measures (include/camo_seg_measures.h):
  python tools/dev/dev_seg_measures_bench.py launches   microseconds per call of camo_seg_histograms and camo_seg_weighted_f at N = 16,
                                                        352 x 352, next to camo_seg_counts on the same bytes (the yardstick: an
                                                        existing kernel that reads the same maps), for a uniform-random, a painted
                                                        (piecewise-constant, 500 regions) and a saturated (binary) prediction
  python tools/dev/dev_seg_measures_bench.py host       cod_measures' host ratios for the 16 tables, and the numpy restatement of
                                                        one image's measures on one host core (needs no GPU)
The library is called directly with every buffer allocated beforehand; every case is warmed up; a window is 200 calls between two
device events, the smallest of five windows is the figure and the largest is printed beside it.  No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import seg_measures_ref as R
from dev_timing import timed
from oracle import rg_features_oracle as FO

N, H, W = 16, 352, 352


def inputs():
    rs = np.random.RandomState(0)
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        cy, cx, r = rs.randint(80, H - 80), rs.randint(80, W - 80), rs.randint(30, 80)
        gt[i][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 255
    uniform = rs.uniform(0, 1, (N, H, W)).astype(np.float32)
    painted = np.stack([rs.uniform(0, 1, 501).astype(np.float32)[FO.voronoi_segments(H, W, 500, 10 + i)] for i in range(N)])
    saturated = (gt > 127).astype(np.float32)
    return gt, {"uniform": uniform, "painted": painted, "saturated": saturated}


def launches():
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    from camouflage_multimodal_amd.seg_measures import gaussian_7x7
    L = _lib.lib()
    gt, preds = inputs()
    g = torch.from_numpy(gt).cuda()
    dev = g.device
    st = _stream_ptr(dev)
    counts = torch.empty(N, 5, dtype=torch.int64, device=dev)
    hist = torch.empty(N, 4, 2, 256, dtype=torch.int32, device=dev)
    split = torch.empty(N, 2, dtype=torch.int32, device=dev)
    sums = torch.empty(N, 3, dtype=torch.int64, device=dev)
    nbytes = L.camo_seg_weighted_f_workspace_bytes(N, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gauss = torch.tensor(gaussian_7x7(), dtype=torch.float64, device=dev)
    for name, pred in preds.items():
        p = torch.from_numpy(pred).cuda()

        def check(rc):
            if rc != 0: raise RuntimeError(L.camo_last_error())
        tc = timed(lambda: check(L.camo_seg_counts(_ptr(p), H * W, _ptr(g), 0.5, N, H, W, _ptr(counts), st)), 200)
        th = timed(lambda: check(L.camo_seg_histograms(_ptr(p), H * W, _ptr(g), N, H, W, _ptr(hist), _ptr(split), st)), 200)
        tw = timed(lambda: check(L.camo_seg_weighted_f(_ptr(p), H * W, _ptr(g), N, H, W, _ptr(gauss), _ptr(ws), nbytes, _ptr(sums), st)), iters=50)
        print(f"N = {N}, {H} x {W}, {name:9s}: camo_seg_counts {tc[0]:.1f} us (up to {tc[1]:.1f}), camo_seg_histograms {th[0]:.1f} us (up to {th[1]:.1f}), "
              f"camo_seg_weighted_f {tw[0]:.1f} us (up to {tw[1]:.1f}) per call", flush=True)


def host():
    from camouflage_multimodal_amd.seg_measures import cod_measures
    gt, preds = inputs()
    hist, split = R.table(preds["painted"], gt)
    t0 = time.perf_counter()
    cod_measures(hist.tolist(), split.tolist(), H, W)
    t1 = time.perf_counter()
    R.measures(preds["painted"][0], gt[0])
    t2 = time.perf_counter()
    print(f"cod_measures, {N} tables: {(t1 - t0) * 1e3:.1f} ms; numpy restatement from the pixels, one image: {(t2 - t1) * 1e3:.1f} ms (one host core)", flush=True)


if __name__ == "__main__":
    {"launches": launches, "host": host}[sys.argv[1]]()
