"""Developer aid / measurement of the edge-aware refinement (include/camo_guided.h):
  python tools/dev/dev_guided_bench.py filter   microseconds per call of camo_guided_filter at 256 x 256, r in {8, 32}, C in {1, 3}, N in {1, 16},
                                                next to (a) the bytes its four launches must move at the measured streaming rate and (b) the same
                                                filter composed in torch in FLOAT64 on the same device (avg_pool2d with count_include_pad=False and
                                                torch.linalg.solve; float32 does not meet the bound), with the largest difference between the two
  python tools/dev/dev_guided_bench.py apply    camo_guided_apply on 16 images of 600 x 800 from 256 x 256 coefficients, next to (a) its bytes and
                                                (b) resize_to_sizes of the C + 1 planes followed by torch elementwise operations
  python tools/dev/dev_guided_bench.py ragged   detect_camouflage_ragged on 16 images of 600 x 800 with and without refine=True (random weights)
The library is called with every buffer allocated beforehand; every case is warmed up; a window is `iters` calls between two device
events, the smallest of five windows is the figure and the largest is printed beside it.  No time is asserted."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from dev_timing import timed

STREAM_BYTES_PER_US = 6.29e6        # tools/dev/microbench/stream_bench.hip: the measured float4 copy rate of the MI355X


def filter_bytes(N, H, W, C):
    """What the four launches must read and write: fp32 inputs, double planes between them, fp32 outputs."""
    K = C * (C + 1) // 2 + 2 * C + 1
    per_pixel = (4 * (C + 1) + 8 * K) + (8 * K + 8 * (C + 1)) + 16 * (C + 1) + (8 * (C + 1) + 4 * C + 4 + 4 * (C + 1))
    return N * H * W * per_pixel


def torch_filter(I, p, r, eps):
    """The guided filter as a user would compose it: float64, clipped windows normalised by their own count."""
    import torch
    import torch.nn.functional as F
    I = I.double().permute(0, 3, 1, 2)
    p = p.double().unsqueeze(1)
    N, C, H, W = I.shape
    box = lambda t: F.avg_pool2d(t, 2 * r + 1, 1, r, count_include_pad=False)
    mu, pb = box(I), box(p)
    cov = box(I * p) - mu * pb
    S = box((I.unsqueeze(2) * I.unsqueeze(1)).reshape(N, C * C, H, W)).reshape(N, C, C, H, W) - mu.unsqueeze(2) * mu.unsqueeze(1)
    S = S.permute(0, 3, 4, 1, 2) + eps * torch.eye(C, dtype=torch.float64, device=I.device)
    a = torch.linalg.solve(S, cov.permute(0, 2, 3, 1).unsqueeze(-1)).squeeze(-1).permute(0, 3, 1, 2)
    b = pb - (a * mu).sum(1, keepdim=True)
    return ((box(a) * I).sum(1) + box(b)[:, 0]).clamp(0, 1).float()


def bench_filter():
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    H = W = 256
    for N in (1, 16):
        for C in (1, 3):
            rs = np.random.RandomState(N + C)
            I = torch.from_numpy(rs.rand(N, H, W, C).astype(np.float32)).cuda()
            p = torch.from_numpy((rs.rand(N, H, W) > 0.5).astype(np.float32)).cuda()
            dev, st = I.device, _stream_ptr(I.device)
            nbytes = L.camo_guided_workspace_bytes(N, H, W, C)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            q = torch.empty(N, H, W, device=dev)
            coef = torch.empty(N, C + 1, H, W, device=dev)
            floor = filter_bytes(N, H, W, C) / STREAM_BYTES_PER_US
            for r in (8, 32):
                def call():
                    rc = L.camo_guided_filter(_ptr(I), _ptr(p), H * W, N, H, W, C, r, 1e-4, 1, _ptr(q), _ptr(coef), _ptr(ws), nbytes, st)
                    if rc != 0: raise RuntimeError(L.camo_last_error())
                t = timed(call, 50 if N == 1 else 10, warm=5)
                u = timed(lambda: torch_filter(I, p, r, 1e-4), 5, windows=3, warm=2)
                diff = float((torch_filter(I, p, r, 1e-4) - q).abs().max())
                print(f"filter N = {N:2d}, 256 x 256, C = {C}, r = {r:2d}: {t[0]:.1f} us (up to {t[1]:.1f}) = {t[0] / floor:.1f} x the traffic floor of "
                      f"{floor:.1f} us ({nbytes / 2 ** 20:.0f} MiB workspace); torch float64 {u[0]:.1f} us (up to {u[1]:.1f}) = {u[0] / t[0]:.1f} x; "
                      f"max |difference| {diff:.2e}", flush=True)


def bench_apply():
    import torch
    from camouflage_multimodal_amd import guided_upsample, pack_images, resize_to_sizes
    N, H, W, h, w = 16, 600, 800, 256, 256
    for C in (1, 3):
        rs = np.random.RandomState(C)
        coef = torch.from_numpy(rs.uniform(-2, 2, (N, C + 1, h, w)).astype(np.float32)).cuda()
        packed = pack_images([rs.randint(0, 256, (H, W, C) if C > 1 else (H, W)).astype(np.uint8) for _ in range(N)])
        floor = N * (H * W * (C + 4) + (C + 1) * h * w * 4) / STREAM_BYTES_PER_US
        native = packed.data.view(N, H, W, C)

        def composed():
            planes, _ = resize_to_sizes(coef, [(H, W)] * N, "bilinear")
            up = torch.stack(planes).double()
            g = native.permute(0, 3, 1, 2).double() / 255.0
            return ((up[:, :C] * g).sum(1) + up[:, C]).clamp(0, 1).float()
        t = timed(lambda: guided_upsample(coef, packed), 20, warm=5)
        u = timed(composed, 5, windows=3, warm=2)
        diff = float((composed() - guided_upsample(coef, packed)[1].view(N, H, W)).abs().max())
        print(f"apply N = {N}, 256 x 256 -> {H} x {W}, C = {C}: {t[0]:.1f} us (up to {t[1]:.1f}) per call (with the table upload) = {t[0] / floor:.1f} x the "
              f"traffic floor of {floor:.1f} us; resize_to_sizes + torch {u[0]:.1f} us (up to {u[1]:.1f}) = {u[0] / t[0]:.1f} x; max |difference| {diff:.2e}",
              flush=True)


def bench_ragged():
    import time
    import torch
    from camouflage_multimodal_amd import RegionGraphGNN, detect_camouflage_ragged, pack_images
    torch.manual_seed(0)
    m = RegionGraphGNN().cuda().eval()
    rs = np.random.RandomState(0)
    packed = pack_images([rs.randint(0, 256, (600, 800, 3)).astype(np.uint8) for _ in range(16)])
    for refine in (None, True):
        def call():
            detect_camouflage_ragged(m, packed, refine=refine)
            torch.cuda.synchronize()
        for _ in range(2): call()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)
        print(f"detect_camouflage_ragged, 16 images of 600 x 800, refine = {refine}: {min(ts) * 1e3:.1f} ms (up to {max(ts) * 1e3:.1f}), host clock "
              f"around a call that ends in a synchronise", flush=True)


if __name__ == "__main__":
    {"filter": bench_filter, "apply": bench_apply, "ragged": bench_ragged}[sys.argv[1]]()
