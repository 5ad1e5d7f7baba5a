"""Developer aid / measurement of the region-graph detector (include/camo_rg_detect.h).  One step per process, so that a caller can
give each its own time limit and stop at the first failure:
  python tools/dev/dev_rg_detect_bench.py launches   microseconds per 256 x 256 image with 500 regions at N = 1 and N = 16 for the
                                                     heads, paint and counts calls alone (node embeddings, label maps and masks
                                                     resident on the device; the output allocations of the calls included)
  python tools/dev/dev_rg_detect_bench.py detect     detect_camouflage_batch end to end (images -> maps and metrics) at N = 1, 16
  python tools/dev/dev_rg_detect_bench.py host       the numpy restatement (tests/rg_detect_ref.py) of heads + paint + counts for
                                                     one such image on one host core (needs no GPU)
Inputs are resident on the device, every shape is warmed up, and each window ends in a device synchronise.  No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rg_detect_ref as R
from oracle import rg_features_oracle as FO


def inputs(n_images):
    rs = np.random.RandomState(0)
    segs = np.stack([FO.voronoi_segments(256, 256, 500, 10 + i) for i in range(n_images)]).astype(np.int32)
    rmap, off = R.region_map_of(segs, 501)
    emb = np.maximum(rs.standard_normal((int(off[-1]), 128)), 0).astype(np.float32)
    gt = (rs.uniform(size=(n_images, 256, 256)) > 0.7).astype(np.uint8) * 255
    return segs, rmap, off, emb, gt


def timed(fn, iters):
    import torch
    for _ in range(5): fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):                                   # three windows: the smallest is the figure
        t0 = time.perf_counter()
        for _ in range(iters): fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / iters)
    return best


def launches():
    import torch
    from camouflage_multimodal_amd import RegionGraphGNN, paint_regions, segmentation_counts
    torch.manual_seed(1)
    m = RegionGraphGNN().cuda().eval()
    segs, rmap, off, emb, gt = inputs(16)
    for n in (1, 16):
        s, r, g = (torch.from_numpy(a[:n]).cuda() for a in (segs, rmap, gt))
        o = [int(v) for v in off[:n + 1]]
        ot = torch.tensor(o, dtype=torch.int32, device="cuda")
        e = torch.from_numpy(emb[:o[-1]]).cuda()
        probs = m.node_heads(e)[1]
        maps = paint_regions(probs, s, r, ot)
        th = timed(lambda: m.node_heads(e), 200)
        tp = timed(lambda: paint_regions(probs, s, r, ot), 200)
        tc = timed(lambda: segmentation_counts(maps[:, 0], g), 200)
        print(f"launches N = {n:2d} ({o[-1]} nodes): heads {th * 1e6:.1f} us, paint {tp * 1e6:.1f} us, counts {tc * 1e6:.1f} us per call = "
              f"{(th + tp + tc) / n * 1e6:.1f} us per image", flush=True)


def detect():
    import torch
    import slic_ref as SR
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage_batch
    torch.manual_seed(1)
    m = RegionGraphGNN().cuda().eval()
    imgs = np.stack([SR.blob_image(256, 256, 3 + (i % 4)) if i % 2 == 0 else SR.noise_image(256, 256, 4 + (i % 4)) for i in range(16)])
    gt = torch.from_numpy((np.random.RandomState(0).uniform(size=(16, 256, 256)) > 0.7).astype(np.uint8) * 255).cuda()
    d = torch.from_numpy(imgs).cuda()
    for n in (1, 16):
        t = timed(lambda: detect_camouflage_batch(m, d[:n], gt[:n]), 20)
        print(f"detect_camouflage_batch N = {n:2d}: {t * 1e6:.0f} us per call = {t / n * 1e6:.0f} us per image", flush=True)


def host():
    segs, rmap, off, emb, gt = inputs(1)
    p = R.make_head_params(0)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        probs = R.probabilities(R.heads(p, emb), 2).astype(np.float32)
        maps = R.paint(probs, segs, rmap, off)
        R.counts(maps[:, 0], gt)
        best = min(best, time.perf_counter() - t0)
    print(f"numpy restatement, one 256 x 256 image with {int(off[-1])} regions, one host core: {best * 1e6:.0f} us", flush=True)


if __name__ == "__main__":
    {"launches": launches, "detect": detect, "host": host}[sys.argv[1]]()
