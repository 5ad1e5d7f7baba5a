"""Developer aid / measurement of the instance extraction (include/camo_instances.h):
  python tools/dev/dev_instances_bench.py launches   microseconds per call of camo_instances at N = 16 of 256 x 256 (the working size)
                                                     and at one 1024 x 1024, for a blob-like mask (a few discs with pinholes) and for
                                                     uniform noise at density 0.5, each with and without fill_holes, connectivity 8;
                                                     next to each time its ratio to the call's traffic floor -- 4 B/pixel read and
                                                     5 B/pixel written at the measured copy bandwidth, 6.29 TB/s -- and the launch count;
                                                     `launches 16 blobs` runs one batch size and one content only (for a profiler)
  python tools/dev/dev_instances_bench.py host       the numpy restatement of one 256 x 256 image on one host core (needs no GPU)
The library is called directly with every buffer allocated beforehand; every case is warmed up; a window is 200 calls between two
device events (50 at 1024 x 1024), the smallest of five windows is the figure and the largest is printed beside it.  The outputs of
every timed case are checked against the restatement for the first image.  No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import instances_ref as R
from dev_timing import timed

SIZES = ((16, 256, 256, 200), (1, 1024, 1024, 50))
COPY_BYTES_PER_US = 6.29e6          # measured float4 copy bandwidth of the MI355X
LAUNCHES = {False: 8, True: 11}     # include/camo_instances.h


def inputs(N, H, W):
    rs = np.random.RandomState(N * 7 + H)
    yy, xx = np.mgrid[:H, :W]
    blobs = rs.uniform(0, 0.45, (N, H, W)).astype(np.float32)
    for i in range(N):
        for _ in range(3):
            cy, cx, r = rs.randint(H // 8, H - H // 8), rs.randint(W // 8, W - W // 8), rs.randint(H // 16, H // 4)
            disc = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
            blobs[i][disc] = rs.uniform(0.55, 1.0, int(disc.sum())).astype(np.float32)
        ys, xs = rs.randint(0, H, H // 2), rs.randint(0, W, H // 2)      # pinholes and specks
        blobs[i, ys, xs] = 1.0 - blobs[i, ys, xs]
    noise = rs.uniform(0, 1, (N, H, W)).astype(np.float32)
    return {"blobs": blobs, "noise": noise}


def launches(only_n=None, only_name=None):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    rows = 64
    for N, H, W, iters in SIZES:
        if only_n is not None and N != int(only_n): continue
        floor = N * H * W * 9 / COPY_BYTES_PER_US
        for name, pred in inputs(N, H, W).items():
            if only_name is not None and name != only_name: continue
            p = torch.from_numpy(pred).cuda()
            dev = p.device
            st = _stream_ptr(dev)
            nbytes = L.camo_instances_workspace_bytes(N, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            labels = torch.empty(N, H, W, dtype=torch.int32, device=dev)
            clean = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
            table = torch.empty(N, rows, 8, dtype=torch.int64, device=dev)
            counts = torch.empty(N, 4, dtype=torch.int32, device=dev)
            for fill in (False, True):
                def call():
                    rc = L.camo_instances(_ptr(p), H * W, 0.5, N, H, W, 8, 0, int(fill), rows, _ptr(labels), _ptr(clean), _ptr(table), _ptr(counts),
                                          _ptr(ws), nbytes, st)
                    if rc != 0: raise RuntimeError(L.camo_last_error())
                t = timed(call, iters)
                want = R.instances_image(pred[0], 0.5, 8, 0, fill, rows)
                got = (labels[0].cpu().numpy(), clean[0].cpu().numpy(), table[0].cpu().numpy(), counts[0].cpu().numpy())
                same = all(np.array_equal(a, b) for a, b in zip(got, want))
                print(f"N = {N}, {H} x {W}, {name:5s}, fill_holes {int(fill)}: {t[0]:.1f} us (up to {t[1]:.1f}) per call = {t[0] / floor:.1f} x the traffic floor "
                      f"of {floor:.2f} us, {LAUNCHES[fill]} launches; instances of image 0: {int(counts[0, 0])}, holes {int(counts[0, 2])}; "
                      f"{'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)


def host():
    pred = inputs(1, 256, 256)["blobs"][0]
    t0 = time.perf_counter()
    R.instances_image(pred, 0.5, 8, 0, True)
    print(f"numpy restatement, one 256 x 256 image with fill_holes: {(time.perf_counter() - t0) * 1e3:.0f} ms (one host core)", flush=True)


if __name__ == "__main__":
    {"launches": launches, "host": host}[sys.argv[1]](*sys.argv[2:4])
