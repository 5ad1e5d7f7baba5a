"""Developer aid / measurement of the SLIC label maps (include/camo_slic.h): microseconds per 256 x 256 image for slic_segments
(500 segments, inputs resident on the device, allocations of the call included) at N = 1 and N = 16, and the numpy / scipy
reference (tests/slic_ref.py, float64) on one core beside it.
  python tools/dev/dev_slic_bench.py"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import slic_ref as R
from camouflage_multimodal_amd import slic_segments

imgs = np.stack([R.blob_image(256, 256, 3 + (i % 4)) if i % 2 == 0 else R.noise_image(256, 256, 4 + (i % 4)) for i in range(16)])
t0 = time.perf_counter(); R.slic(imgs[1], 500); cpu = time.perf_counter() - t0
for n in (1, 16):
    d = torch.from_numpy(imgs[:n]).cuda()
    for _ in range(5): lab, cnt = slic_segments(d, 500, return_counts=True)
    torch.cuda.synchronize()
    it = 50
    t0 = time.perf_counter()
    for _ in range(it): lab = slic_segments(d, 500)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / it
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(it): lab = slic_segments(d, 500)
    ev[1].record(); torch.cuda.synchronize()
    print(f"slic N = {n:2d}: {dt * 1e6:.0f} us per call = {dt / n * 1e6:.1f} us per image by the host clock, {ev[0].elapsed_time(ev[1]) / it / n * 1e3:.1f} us per image "
          f"by device events; labels per image {(cnt[:, 0] - 1).tolist()}, oversized {cnt[:, 1].tolist()}; reference on one host core {cpu * 1e3:.0f} ms")
