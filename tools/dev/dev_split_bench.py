"""Developer aid / measurement of the instance splitter (include/camo_split.h):
  python tools/dev/dev_split_bench.py launches   microseconds per call of camo_split_instances at N = 16 of 256 x 256 (the working size)
                                                 and at one 1024 x 1024, on the label maps camo_instances makes of dev_instances_bench.py's
                                                 blob-like mask and uniform noise (connectivity 8; min_area raised in powers of two until
                                                 no image holds more than CAMO_IM_MAX_IDS ids), at the default parameters and with the
                                                 prediction given; beside each time camo_instances' own on the same map, the ratio to the
                                                 call's traffic floor -- 4 B/pixel of labels and 4 B/pixel of prediction read, 4 B/pixel
                                                 written, at the measured copy bandwidth, 6.29 TB/s -- and the launch count;
                                                 `launches 16 blobs` runs one batch size and one content only (for a profiler)
  python tools/dev/dev_split_bench.py host       the numpy restatement of one 256 x 256 image on one host core (needs no GPU)
The library is called directly with every buffer allocated beforehand; every case is warmed up; a window is 200 calls between two
device events (50 at 1024 x 1024), the smallest of five windows is the figure and the largest is printed beside it.  At 256 x 256 the
outputs of every timed case are checked against the restatement for the first image (its brute force is too slow for 1024 x 1024:
there the foreground and the counts' sums are checked).  No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref as IR
import split_ref as R
from dev_instances_bench import COPY_BYTES_PER_US, SIZES, inputs
from dev_timing import timed

ROWS = 64


def label_maps(pred):
    """(labels int32 [N, H, W] on the device, min_area) of camo_instances on ``pred`` with at most CAMO_IM_MAX_IDS ids an image."""
    import torch
    from camouflage_multimodal_amd import _lib, mask_instances
    p = torch.from_numpy(pred).cuda()
    min_area = 0
    while True:
        out = mask_instances(p, 0.5, 8, min_area, False, ROWS)
        if int(out["counts"][:, 0].max()) <= _lib.IM_MAX_IDS:
            return p, out["labels"], min_area
        min_area = max(2 * min_area, 2)


def launches(only_n=None, only_name=None):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    for N, H, W, iters in SIZES:
        if only_n is not None and N != int(only_n): continue
        floor = N * H * W * 12 / COPY_BYTES_PER_US
        for name, pred in inputs(N, H, W).items():
            if only_name is not None and name != only_name: continue
            p, labels, min_area = label_maps(pred)
            dev = p.device
            st = _stream_ptr(dev)
            nbytes = L.camo_split_workspace_bytes(N, H, W, 4)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            out = torch.empty(N, H, W, dtype=torch.int32, device=dev)
            table = torch.empty(N, ROWS, 8, dtype=torch.int64, device=dev)
            counts = torch.empty(N, 4, dtype=torch.int32, device=dev)
            ibytes = L.camo_instances_workspace_bytes(N, H, W)
            iws = torch.empty(ibytes, dtype=torch.uint8, device=dev)
            ilabels, iclean, icounts = torch.empty_like(out), torch.empty(N, H, W, dtype=torch.uint8, device=dev), torch.empty_like(counts)

            def call():
                rc = L.camo_split_instances(_ptr(labels), _ptr(p), H * W, N, H, W, 7, 10, 0, 4, ROWS, _ptr(out), _ptr(table), _ptr(counts), _ptr(ws), nbytes, st)
                if rc != 0: raise RuntimeError(L.camo_last_error())

            def instances():
                rc = L.camo_instances(_ptr(p), H * W, 0.5, N, H, W, 8, min_area, 0, ROWS, _ptr(ilabels), _ptr(iclean), _ptr(table), _ptr(icounts), _ptr(iws), ibytes, st)
                if rc != 0: raise RuntimeError(L.camo_last_error())
            ti = timed(instances, iters)
            t = timed(call, iters)
            c = counts.cpu().numpy()
            if H * W <= 256 * 256:
                want = R.split_image(labels[0].cpu().numpy(), pred[0], max_instances=ROWS)
                same = all(np.array_equal(a, b) for a, b in zip((out[0].cpu().numpy(), table[0].cpu().numpy(), c[0]), want[:3]))
                verdict = f"{'equal to' if same else 'DIFFERENT FROM'} the restatement"
            else:
                ok = bool(((out > 0) == (labels > 0)).all()) and int(out.max()) == int(c[:, 0].max())
                verdict = f"foreground and id range {'kept' if ok else 'WRONG'} (the restatement is not run at this size)"
            print(f"N = {N}, {H} x {W}, {name:5s} (min_area {min_area}): {t[0]:.1f} us (up to {t[1]:.1f}) per call = {t[0] / floor:.1f} x the traffic floor of "
                  f"{floor:.2f} us, {_lib.SPLIT_LAUNCHES} launches; camo_instances on the same map {ti[0]:.1f} us; image 0: {int(labels[0].max())} ids in, "
                  f"(K', split, dropped, left whole) = {c[0].tolist()}; the batch: {c.sum(axis=0).tolist()}; {verdict}", flush=True)


def host():
    pred = inputs(1, 256, 256)["blobs"][0]
    labels = IR.instances_image(pred, 0.5, 8, 0, False)[0]
    t0 = time.perf_counter()
    R.split_image(labels, pred)
    print(f"numpy restatement, one 256 x 256 image: {(time.perf_counter() - t0) * 1e3:.0f} ms (one host core)", flush=True)


if __name__ == "__main__":
    {"launches": launches, "host": host}[sys.argv[1]](*sys.argv[2:4])
