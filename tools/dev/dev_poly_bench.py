"""Developer aid / measurement of COCO polygon annotations (include/camo_poly.h):
  python tools/dev/dev_poly_bench.py calls     two loads -- (a) 16 images of 256 x 256 with 4 annotations of one 100-vertex polygon each,
                                               (b) one 768 x 1024 image with 20 annotations of 100 vertices: microseconds per call of
                                               camo_poly_decode, every buffer allocated beforehand; the same for camo_rle_decode on the
                                               RLEs of the same masks (the existing way in); the wall time of decode_polygons and of
                                               decode_rles, host work and the upload included; and the numpy restatement
                                               (tests/poly_ref.py) on one host core with the upload of its maps
  python tools/dev/dev_poly_bench.py loop a    one load only, 200 calls of camo_poly_decode (for a kernel trace)
A device window is 200 calls between two device events, the smallest of five windows is the figure and the largest is printed beside
it; a wall time is the smallest of three calls after a warm-up.  The outputs of every timed case are checked against the restatement.
No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import poly_ref as P
import rle_ref as R
from dev_timing import timed

LOADS = {"a": (16, 256, 256, 4), "b": (1, 768, 1024, 20)}
VERTICES = 100


def load(name):
    """per image [(polygons, value)]: stars of VERTICES vertices, radii between a tenth and a third of the image."""
    N, H, W, K = LOADS[name]
    rng = np.random.default_rng(N * 100 + K)
    per = []
    for n in range(N):
        anns = []
        for k in range(K):
            ang = np.sort(rng.uniform(0, 2 * np.pi, VERTICES))
            rad = rng.uniform(0.1, 0.33) * min(H, W) * rng.uniform(0.6, 1.0, VERTICES)
            cx, cy = rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H
            anns.append(([np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1).reshape(-1).tolist()], k + 1))
        per.append(anns)
    return per, N, H, W


def wall(fn, repeats=3):
    import torch
    fn()
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e6
        best = dt if best is None else min(best, dt)
    return best, out


def prepared_poly(per, N, H, W):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    xy, po, apo, img, val = P.arrays(per)
    A, Pn, V = len(img), len(po) - 1, len(xy)
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (xy, po, apo, img, val)]
    nbytes = L.camo_poly_decode_workspace_bytes(N, H, W, A, Pn, V)
    labels, area = torch.empty(N, H, W, dtype=torch.int32, device="cuda"), torch.empty(A, dtype=torch.int64, device="cuda")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _stream_ptr(labels.device)

    def call():
        rc = L.camo_poly_decode(_ptr(dev[0]), V, _ptr(dev[1]), Pn, _ptr(dev[2]), _ptr(dev[3]), _ptr(dev[4]), A, N, H, W, _ptr(labels), _ptr(area), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return call, labels, (A, Pn, V)


def prepared_rle(rles, N, H, W):
    import torch
    from camouflage_multimodal_amd import _lib, rle as _rle
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    cnts, off, img, val = _rle._annotations(rles, H, W)
    A, total = img.size, cnts.size
    dev = [torch.from_numpy(v).cuda() for v in (cnts, off, img, val)]
    nbytes = L.camo_rle_decode_workspace_bytes(N, H, W, A, total)
    labels, sums = torch.empty(N, H, W, dtype=torch.int32, device="cuda"), torch.empty(A, dtype=torch.int64, device="cuda")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _stream_ptr(labels.device)

    def call():
        rc = L.camo_rle_decode(_ptr(dev[0]), total, _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), A, N, H, W, _ptr(labels), _ptr(sums), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return call, labels, total


def calls():
    import torch
    from camouflage_multimodal_amd import counts_to_string, decode_polygons, decode_rles
    for name in LOADS:
        per, N, H, W = load(name)
        t0 = time.perf_counter()
        want = np.stack([P.label_map(anns, H, W) for anns in per])
        host_us = (time.perf_counter() - t0) * 1e6
        tu, _ = wall(lambda: torch.from_numpy(want).cuda())
        call, labels, (A, Pn, V) = prepared_poly(per, N, H, W)
        t = timed(call, 200)
        same = labels.cpu().numpy().tobytes() == want.tobytes()
        points = sum(len(P.boundary_points(*P.scaled_vertices(p))[0]) for anns in per for polys, _ in anns for p in polys)
        print(f"load ({name}): N = {N}, {H} x {W}, {A} annotations, {V} vertices, {points} boundary points: camo_poly_decode {t[0]:.1f} us (up to {t[1]:.1f}) "
              f"per call, 4 launches; {'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)
        tw, got = wall(lambda: decode_polygons(per, H, W))
        print(f"        decode_polygons {tw:.0f} us wall (host checks, one upload, the call); {'equal' if got.cpu().numpy().tobytes() == want.tobytes() else 'DIFFERENT'}", flush=True)
        # the existing way in: every annotation's own mask as an RLE (rasterised on the host beforehand, not timed)
        rles = [[({"size": [H, W], "counts": counts_to_string(R.mask_counts(P.label_map([(polys, 1)], H, W) > 0))}, v) for polys, v in anns] for anns in per]
        call, back, total = prepared_rle(rles, N, H, W)
        t = timed(call, 200)
        print(f"        camo_rle_decode on the RLEs of the same masks {t[0]:.1f} us (up to {t[1]:.1f}) per call, 2 launches, {total} counts; "
              f"{'equal' if back.cpu().numpy().tobytes() == want.tobytes() else 'DIFFERENT'}", flush=True)
        tw, got = wall(lambda: decode_rles(rles, H, W))
        print(f"        decode_rles {tw:.0f} us wall; {'equal' if got.cpu().numpy().tobytes() == want.tobytes() else 'DIFFERENT'}", flush=True)
        print(f"        numpy restatement on one host core {host_us:.0f} us (one run), upload of its maps {tu:.0f} us", flush=True)


def loop(name):
    import torch
    per, N, H, W = load(name)
    call, _, _ = prepared_poly(per, N, H, W)
    for _ in range(200): call()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"calls": calls, "loop": loop}[sys.argv[1]](*sys.argv[2:3])
