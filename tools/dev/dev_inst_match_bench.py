"""Developer aid / measurement of instance matching (include/camo_inst_match.h):
  python tools/dev/dev_inst_match_bench.py calls           microseconds per call of camo_inst_match at 256 x 256, P = G = 64, the COCO
                                                           thresholds, N = 1 and N = 16, for blob-like label maps (discs against
                                                           their shifted copies) and for the 40-by-37 pair pattern (a new pair at
                                                           every pixel: the overlap launch's worst case); then the host route the
                                                           call replaces -- both label maps copied to the host, the overlap table
                                                           by np.bincount -- for the same maps
  python tools/dev/dev_inst_match_bench.py loop 16 blobs   one batch size and one content only, 200 calls (for a kernel trace)
The library is called directly with every buffer allocated beforehand; every case is warmed up; a window is 200 calls between two
device events, the smallest of five windows is the figure and the largest is printed beside it.  The outputs of every timed case are
checked against the restatement for the first image.  No time is asserted."""
import os, sys, time
import ctypes
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import inst_match_ref as R
from dev_timing import timed

H = W = 256
P = G = 64
LAUNCHES = 4                        # include/camo_inst_match.h


def inputs(N):
    rs = np.random.RandomState(N * 7 + 1)
    yy, xx = np.mgrid[:H, :W]
    blobs = np.zeros((N, H, W), np.int32)
    for i in range(N):
        for k in range(20):
            cy, cx, r = rs.randint(H // 8, H - H // 8), rs.randint(W // 8, W - W // 8), rs.randint(H // 32, H // 8)
            blobs[i][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    pairs = np.broadcast_to(((xx + yy) % 40 + 1).astype(np.int32), (N, H, W)).copy()
    pairs_gt = np.broadcast_to(((xx * 3 + yy) % 37 + 1).astype(np.int32), (N, H, W)).copy()
    table = np.zeros((N, P, 8), np.int64)
    table[..., 0] = rs.randint(1, 4000, (N, P))
    table[..., 7] = (table[..., 0] * rs.uniform(128, 255, (N, P))).astype(np.int64)
    return {"blobs": (blobs, np.roll(blobs, (3, 5), (1, 2))), "pairs": (pairs, pairs_gt)}, table


def prepared(N, pred, gt, table):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    pl, gl, tab = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(table).cuda()
    st = _stream_ptr(pl.device)
    T = len(R.COCO)
    nums = (ctypes.c_int32 * T)(*range(10, 20))
    nbytes = L.camo_inst_match_workspace_bytes(N, H, W, P, G, T)
    i32 = dict(dtype=torch.int32, device=pl.device)
    out = {"inter": torch.empty(N, P + 1, G + 1, **i32), "pred_rows": torch.empty(N, P, 4, **i32), "gt_area": torch.empty(N, G, **i32),
           "match": torch.empty(N, T, P, **i32), "gt_match": torch.empty(N, T, G, **i32), "counts": torch.empty(N, 4, **i32)}
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pl.device)

    def call():
        rc = L.camo_inst_match(_ptr(pl), _ptr(gl), N, H, W, P, G, _ptr(tab), P, nums, 20, T, *(_ptr(v) for v in out.values()), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return call, out, (pl, gl)


def calls():
    import torch
    for N in (1, 16):
        maps, table = inputs(N)
        for name, (pred, gt) in maps.items():
            call, out, (pl, gl) = prepared(N, pred, gt, table)
            t = timed(call, 200)
            want = R.match_image(pred[0], gt[0], P, G, table[0], R.COCO)
            same = all(np.array_equal(out[k][0].cpu().numpy(), want[k]) for k in want)
            print(f"N = {N:2d}, {H} x {W}, P = G = {P}, {name:5s}: {t[0]:.1f} us (up to {t[1]:.1f}) per call, {LAUNCHES} launches; ids in use "
                  f"{out['counts'][0, 2:].tolist()}, matched at 0.5: {int((out['match'][0, 0] > 0).sum())}; "
                  f"{'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)
            best = None
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a, b = pl.cpu().numpy(), gl.cpu().numpy()
                tables = [np.bincount(a[i].ravel().astype(np.int64) * (G + 1) + b[i].ravel(), minlength=(P + 1) * (G + 1)) for i in range(N)]
                dt = (time.perf_counter() - t0) * 1e6
                best = dt if best is None else min(best, dt)
            assert np.array_equal(tables[0].reshape(P + 1, G + 1), want["inter"])
            print(f"        host route, {name:5s}: {best:.0f} us (two copies and np.bincount, no matching; the smallest of five)", flush=True)


def loop(n, name):
    import torch
    maps, table = inputs(int(n))
    call, _, _ = prepared(int(n), *maps[name], table)
    for _ in range(200): call()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"calls": calls, "loop": loop}[sys.argv[1]](*sys.argv[2:4])
