"""Developer aid / measurement of the region-graph fine-tuner at 16 and at 128 images of 256 x 256:
node_targets_from_masks alone (against its algorithmic traffic N H W (4 + 1) bytes over the HBM roof), RegionGraphFineTuner.step on a
prepared batch, and step_from_images (superpixels, edge maps, graphs, targets and CSRs rebuilt every step).
  python tools/dev/dev_rg_finetune_bench.py [images_per_batch ...]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, node_targets_from_masks, prepare_finetune_batch

HBM_ROOF = 8.0e12          # bytes / s, the MI355X figure DESIGN.md uses


def timed(fn, it=20, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(it): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / it


def scene(N, H=256, W=256, seed=0):
    """Textured ground with a brighter ellipse per image, and the ellipse as the mask."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.empty((N, H, W, 3), np.float32)
    gt = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        ground = 0.35 + 0.15 * np.sin(yy / rs.uniform(5, 15)) * np.cos(xx / rs.uniform(5, 15)) + rs.uniform(-0.05, 0.05, (H, W))
        cy, cx, ry, rx = rs.uniform(60, 196), rs.uniform(60, 196), rs.uniform(25, 60), rs.uniform(25, 60)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        img[i] = np.stack([ground, 0.9 * ground + 0.03, 0.8 * ground + 0.05], -1)
        img[i][inside] += 0.2
        gt[i][inside] = 255
    return torch.from_numpy(np.clip(img, 0, 1)).cuda(), torch.from_numpy(gt).cuda()


for N in [int(a) for a in sys.argv[1:]] or [16, 128]:
    img, gt = scene(N)
    tuner = RegionGraphFineTuner(RegionGraphGNN().cuda().eval(), lr=1e-4)
    batch = prepare_finetune_batch(img, gt)
    off = batch.graphs.node_offsets
    n = off[-1]
    tg = timed(lambda: node_targets_from_masks(batch.segments, batch.region_map, off, gt), it=100, warm=10)
    st = timed(lambda: tuner.step(batch))
    fi = timed(lambda: tuner.step_from_images(img, gt), it=10, warm=2)
    traffic = N * 256 * 256 * 5
    print(f"{N} images / {n} nodes / {batch.csr[1].shape[0]} CSR entries: node_targets_from_masks {tg * 1e6:.1f} us "
          f"({traffic / HBM_ROOF * 1e6:.2f} us of traffic at the HBM roof = {traffic / HBM_ROOF / tg:.3f} of the call), "
          f"step {st * 1e6:.1f} us, step_from_images {fi * 1e6:.1f} us")
