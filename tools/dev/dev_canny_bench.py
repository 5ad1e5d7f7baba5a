"""Developer aid / measurement of the Canny edge maps (include/camo_canny.h): microseconds per 256 x 256 image for canny_edges
at N = 1 and N = 16 (inputs resident; the call allocates its workspace and outputs and enqueues five launches), the host
reference (tests/canny_ref.py, numpy / scipy.ndimage, float64) on one core beside it.
  python tools/dev/dev_canny_bench.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import canny_ref as R
from camouflage_multimodal_amd import canny_edges

imgs = np.stack([R.grey_image(R.noise_field(256, 256, s)) if s % 2 else R.colour_image(256, 256, s) for s in range(16)])
t0 = time.perf_counter(); ref, _ = R.canny(imgs[1]); cpu = time.perf_counter() - t0
for n in (1, 16):
    d = torch.from_numpy(imgs[:n]).cuda()
    for _ in range(10): e = canny_edges(d)
    torch.cuda.synchronize()
    it = 200
    t0 = time.perf_counter()
    for _ in range(it): e = canny_edges(d)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / it
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(it): e = canny_edges(d)
    ev[1].record(); torch.cuda.synchronize()
    print(f"canny N = {n:2d}: {dt * 1e6:.0f} us per call = {dt / n * 1e6:.1f} us per image by the host clock, {ev[0].elapsed_time(ev[1]) / it / n * 1e3:.1f} us per image "
          f"between device events; {int(e.sum())} edge pixels")
print(f"host reference (float64, one core): {cpu * 1e3:.1f} ms per image; edge pixels of image 1: {int(ref.sum())}")
