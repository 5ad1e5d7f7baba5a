"""Developer aid / measurement of the structure loss on the painted mask (include/camo_rg_pixel_loss.h):
  python tools/dev/dev_pixel_loss_bench.py weights   microseconds per call of camo_rg_pixel_weights at N = 1 and N = 16 of 256 x 256 with
                                                     500 regions (a Voronoi label map, blob-like ground truths), at radius 15 / gain 5 and at
                                                     radius 31 / gain 16; beside each time camo_rg_node_targets' on the same arrays and the
                                                     ratio to the call's traffic floor -- 4 B/pixel of labels and 1 B/pixel of ground truth
                                                     read, at the measured copy bandwidth, 6.29 TB/s; node_w of every timed case is checked
                                                     against the restatement
  python tools/dev/dev_pixel_loss_bench.py step      microseconds per RegionGraphFineTuner.step on a batch prepared from 16 images of
                                                     256 x 256 (n_segments 500, the model's default sizes): without the pixel term -- the
                                                     entry point the step had before, camo_rg_loss_backward -- and with pixel_loss = 1.0,
                                                     alternating, on one CSR pair
The arrays are allocated beforehand; every case is warmed up; a window is 200 calls between two device events, the smallest of five
windows is the figure and the largest is printed beside it.  No time is asserted."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rg_pixel_loss_ref as PR
import rg_targets_ref as TG
from dev_instances_bench import COPY_BYTES_PER_US, inputs
from dev_timing import timed
from oracle import rg_features_oracle as FO

H = W = 256
REGIONS, ITERS = 500, 200


def masks(N):
    return np.where(inputs(N, H, W)["blobs"] > 0.5, 255, 0).astype(np.uint8)


def weights():
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    one = FO.voronoi_segments(H, W, REGIONS, 9)
    for N in (1, 16):
        seg = np.ascontiguousarray(np.broadcast_to(one, (N, H, W))).astype(np.int32)
        rmap, off = TG.compact_region_map(seg, 512)
        gt, n = masks(N), int(off[-1])
        d_seg, d_rmap, d_off, d_gt = (torch.from_numpy(a).cuda() for a in (seg, rmap, off.astype(np.int32), gt))
        st = _stream_ptr(d_seg.device)
        node_w = torch.empty(n, 2, dtype=torch.int64, device="cuda")
        counts = torch.empty(n, 4, dtype=torch.int32, device="cuda")
        mt, it, et = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, device="cuda")
        floor = N * H * W * 5 / COPY_BYTES_PER_US

        def targets():
            rc = L.camo_rg_node_targets(_ptr(d_seg), _ptr(d_rmap), _ptr(d_off), _ptr(d_gt), None, None, N, H, W, 512, n, 0, 1, _ptr(counts), _ptr(mt),
                                        _ptr(it), _ptr(et), st)
            if rc != 0: raise RuntimeError(L.camo_last_error())
        tt = timed(targets, ITERS)
        for radius, gain in ((15, 5), (31, 16)):
            def call():
                rc = L.camo_rg_pixel_weights(_ptr(d_seg), _ptr(d_rmap), _ptr(d_off), _ptr(d_gt), N, H, W, 512, n, radius, gain, _ptr(node_w), st)
                if rc != 0: raise RuntimeError(L.camo_last_error())
            t = timed(call, ITERS)
            same = np.array_equal(node_w.cpu().numpy(), PR.node_weights(seg, rmap, off, gt, radius, gain))
            print(f"N = {N}, {H} x {W}, {n} nodes, radius {radius}, gain {gain}: {t[0]:.1f} us (up to {t[1]:.1f}) per call = {t[0] / floor:.1f} x the "
                  f"traffic floor of {floor:.2f} us, 2 launches; camo_rg_node_targets on the same arrays {tt[0]:.1f} us; node_w "
                  f"{'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)


def step():
    import torch
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, prepare_finetune_batch
    N = 16
    gt = masks(N)
    rs = np.random.RandomState(5)
    img = np.clip(0.3 + 0.4 * (gt[..., None] > 127) + rs.uniform(-0.15, 0.15, (N, H, W, 3)), 0, 1).astype(np.float32)
    batch = prepare_finetune_batch(torch.from_numpy(img).cuda(), torch.from_numpy(gt).cuda(), n_segments=REGIONS, pixel_loss=True)
    tuners = {}
    for name, w in (("without the pixel term (camo_rg_loss_backward)", 0.0), ("with pixel_loss = 1.0 (camo_rg_loss_backward_pixel)", 1.0)):
        torch.manual_seed(1)
        tuners[name] = RegionGraphFineTuner(RegionGraphGNN().cuda(), lr=1e-5, pixel_loss=w)
    for rnd in range(2):                                             # alternating: the second round is the figure to read
        for name, tuner in tuners.items():
            t = timed(lambda: tuner.step(batch), ITERS)
            out = {k: round(float(v), 4) for k, v in tuner.step(batch).items()}
            print(f"round {rnd + 1}, N = {N}, {batch.graphs.x.shape[0]} nodes, {batch.csr[1].shape[0]} CSR entries, step {name}: {t[0]:.1f} us "
                  f"(up to {t[1]:.1f}); {out}", flush=True)


if __name__ == "__main__":
    {"weights": weights, "step": step}[sys.argv[1]]()
