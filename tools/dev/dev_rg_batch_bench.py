"""Developer aid / measurement of the batched region-graph construction (include/camo_rg_batch.h).  One step per process, so that
a caller can give each its own time limit and stop at the first failure:
  python tools/dev/dev_rg_batch_bench.py construct   microseconds per 256 x 256 image with 500 regions at N = 1, 4, 16 for
                                                     create_region_graphs_from_segments (sizes read-back and allocations of the
                                                     call included, label_bound and the edge maps given), beside
                                                     create_region_graph_from_segments called N times
  python tools/dev/dev_rg_batch_bench.py predict     image -> prediction per image at N = 16: predict_batch_from_images beside a
                                                     loop of predict_from_image (f32 and bf16 fusion model)
Inputs are resident on the device, every shape is warmed up, and each window ends in a device synchronise."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import rg_features_oracle as RO
from camouflage_multimodal_amd import (RegionGraphGNN, build_multimodal_model, create_region_graph_from_segments,
                                       create_region_graphs_from_segments, predict_batch_from_images, predict_from_image)


def timed(fn, iters):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):                                   # three windows: the spread is printed, the smallest is the figure
        t0 = time.perf_counter()
        for _ in range(iters): fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / iters)
    return best


def construct():
    rs = np.random.RandomState(0)
    segs = np.stack([RO.voronoi_segments(256, 256, 500, 10 + i) for i in range(16)]).astype(np.int32)
    imgs = rs.uniform(0, 1, (16, 256, 256, 3)).astype(np.float32)
    can = rs.uniform(0, 1, (16, 256, 256)) > 0.85
    for n in (1, 4, 16):
        i, s, c = (torch.from_numpy(a[:n]).cuda() for a in (imgs, segs, can))
        new = timed(lambda: create_region_graphs_from_segments(i, s, c, label_bound=501), 100)
        old = timed(lambda: [create_region_graph_from_segments(i[k], s[k], c[k]) for k in range(n)], max(100 // n, 10))
        g, _ = create_region_graphs_from_segments(i, s, c, label_bound=501)
        print(f"construction N = {n:2d}: batched call {new * 1e6:.0f} us = {new / n * 1e6:.1f} us per image; per-image call x N {old * 1e6:.0f} us = "
              f"{old / n * 1e6:.1f} us per image; nodes {g.node_offsets[-1]}, directed edges {g.edge_offsets[-1]}", flush=True)


def predict():
    import slic_ref as R
    imgs = np.stack([R.blob_image(256, 256, 3 + (i % 4)) if i % 2 == 0 else R.noise_image(256, 256, 4 + (i % 4)) for i in range(16)])
    d = torch.from_numpy(imgs).cuda()
    torch.manual_seed(1)
    rgm = RegionGraphGNN().cuda().eval()
    kg = {f"cat{i:02d}": torch.randn(1, 128) for i in range(13)}
    for precision in ("f32", "bf16"):
        fm = build_multimodal_model({}).cuda().eval().set_precision(precision)
        new = timed(lambda: predict_batch_from_images(fm, rgm, d, kg, "cuda"), 20)
        old = timed(lambda: [predict_from_image(fm, rgm, d[k], kg, "cuda") for k in range(16)], 5)
        print(f"image -> prediction N = 16 ({precision}): predict_batch_from_images {new / 16 * 1e6:.0f} us per image; loop of predict_from_image "
              f"{old / 16 * 1e6:.0f} us per image", flush=True)


if __name__ == "__main__":
    {"construct": construct, "predict": predict}[sys.argv[1]]()
