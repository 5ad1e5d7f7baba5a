"""Developer aid / measurement of Boundary IoU (include/camo_boundary.h):
  python tools/dev/dev_boundary_bench.py calls             microseconds per call of camo_boundary_labels at N = 1 and 16 -- 256 x 256 with
                                                           d = 7, 768 x 1024 with d = 26 and with d = 1 (the cost must not follow d) --
                                                           with the host route beside it (the map copied to the host, scipy's
                                                           binary erosion of the padded mask per label); then camo_boundary_match
                                                           next to camo_inst_match on dev_inst_match_bench.py's "blobs" and "pairs"
  python tools/dev/dev_boundary_bench.py loop labels 16    one case only, 200 calls (for a kernel trace): labels | labels_big | match
The library is called directly with every buffer allocated beforehand; every case is warmed up with 20 calls; a window is 200 calls
between two device events, the smallest of five windows is the figure and the largest is printed beside it.  The outputs of image 0
are checked in the same run: against the restatement (tests/boundary_ref.py) at 256 x 256, against the host route at 768 x 1024
(which tests/test_boundary.py holds to the restatement).  No time is asserted."""
import os, sys, time
import ctypes
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_ref as B
import inst_match_ref as R
from dev_inst_match_bench import inputs as match_inputs
from dev_timing import timed

P = G = 64
SHAPES = {"labels": (256, 256, 7), "labels_big": (768, 1024, 26), "labels_big_d1": (768, 1024, 1)}


def blobs(N, H, W):
    rs = np.random.RandomState(N * 7 + H)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N, H, W), np.int32)
    for i in range(N):
        for k in range(20):
            cy, cx, r = rs.randint(H // 8, H - H // 8), rs.randint(W // 8, W - W // 8), rs.randint(H // 32, H // 4)
            out[i][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = k + 1
    return out


def host_route(lab, d):
    """The boundary map of one [H, W] label map as the Boundary IoU API makes it, scipy in the place of cv2."""
    from scipy import ndimage
    out = np.zeros_like(lab)
    for k in np.unique(lab[lab > 0]):
        m = lab == k
        out[m & ~ndimage.binary_erosion(np.pad(m, 1), np.ones((3, 3)), iterations=d, border_value=1)[1:-1, 1:-1]] = k
    return out


def prepared_labels(lab, d):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    N, H, W = lab.shape
    dev = torch.from_numpy(lab).cuda()
    out = torch.empty_like(dev)
    nbytes = L.camo_boundary_labels_workspace_bytes(N, H, W, d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev.device)
    st = _stream_ptr(dev.device)

    def call():
        rc = L.camo_boundary_labels(_ptr(dev), N, H, W, d, _ptr(out), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return call, out, dev


def prepared_match(N, pred, gt, pb, gb, table, boundary):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    H, W = pred.shape[1:]
    t = [torch.from_numpy(a).cuda() for a in (pred, gt, pb, gb)]
    tab = torch.from_numpy(table).cuda()
    st = _stream_ptr(tab.device)
    T = len(R.COCO)
    nums = (ctypes.c_int32 * T)(*range(10, 20))
    i32 = dict(dtype=torch.int32, device=tab.device)
    if boundary:
        nbytes = L.camo_boundary_match_workspace_bytes(N, H, W, P, G, T)
        out = {"inter": torch.empty(N, P + 1, G + 1, **i32), "inter_bd": torch.empty(N, P + 1, G + 1, **i32), "pred_rows": torch.empty(N, P, 6, **i32),
               "gt_area": torch.empty(N, G, 2, **i32), "match": torch.empty(N, T, P, **i32), "gt_match": torch.empty(N, T, G, **i32),
               "counts": torch.empty(N, 4, **i32)}
    else:
        nbytes = L.camo_inst_match_workspace_bytes(N, H, W, P, G, T)
        out = {"inter": torch.empty(N, P + 1, G + 1, **i32), "pred_rows": torch.empty(N, P, 4, **i32), "gt_area": torch.empty(N, G, **i32),
               "match": torch.empty(N, T, P, **i32), "gt_match": torch.empty(N, T, G, **i32), "counts": torch.empty(N, 4, **i32)}
    ws = torch.empty(nbytes, dtype=torch.uint8, device=tab.device)

    def call():
        if boundary:
            rc = L.camo_boundary_match(*(_ptr(v) for v in t), N, H, W, P, G, _ptr(tab), P, nums, 20, T, *(_ptr(v) for v in out.values()), _ptr(ws), nbytes, st)
        else:
            rc = L.camo_inst_match(_ptr(t[0]), _ptr(t[1]), N, H, W, P, G, _ptr(tab), P, nums, 20, T, *(_ptr(v) for v in out.values()), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return call, out, t


def match_case(N, name, d=7):
    maps, table = match_inputs(N)
    pred, gt = maps[name]
    return pred, gt, np.stack([host_route(m, d) for m in pred]), np.stack([host_route(m, d) for m in gt]), table


def calls():
    import torch
    for case, (H, W, d) in SHAPES.items():
        for N in (1, 16):
            lab = blobs(N, H, W)
            call, out, dev = prepared_labels(lab, d)
            t = timed(call, 200)
            best = None
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                want = host_route(dev[0].cpu().numpy(), d)
                dt = (time.perf_counter() - t0) * 1e6
                best = dt if best is None else min(best, dt)
            same = np.array_equal(out[0].cpu().numpy(), want) and (H > 256 or np.array_equal(want, B.boundary_labels_ref(lab[0], d)))
            print(f"camo_boundary_labels N = {N:2d}, {H} x {W}, d = {d:2d}: {t[0]:.1f} us (up to {t[1]:.1f}) per call, 2 launches; boundary pixels of image 0: "
                  f"{int((want > 0).sum())} of {int((lab[0] > 0).sum())}; {'equal to' if same else 'DIFFERENT FROM'} the "
                  f"{'restatement and the ' if H <= 256 else ''}host route; host route, ONE image: {best:.0f} us (copy and scipy erosion per label)", flush=True)
    for N in (1, 16):
        for name in ("blobs", "pairs"):
            pred, gt, pb, gb, table = match_case(N, name)
            plain, _, _ = prepared_match(N, pred, gt, pb, gb, table, False)
            call, out, _ = prepared_match(N, pred, gt, pb, gb, table, True)
            tp, tb = timed(plain, 200), timed(call, 200)
            want = B.boundary_match_image(pred[0], gt[0], pb[0], gb[0], P, G, table[0], R.COCO)
            same = all(np.array_equal(out[k][0].cpu().numpy(), want[k]) for k in want)
            print(f"camo_boundary_match N = {N:2d}, 256 x 256, d = 7, P = G = {P}, {name:5s}: {tb[0]:.1f} us (up to {tb[1]:.1f}) per call, 7 launches; "
                  f"camo_inst_match in the same run: {tp[0]:.1f} us (up to {tp[1]:.1f}); matched at 0.5: {int((out['match'][0, 0] > 0).sum())}; "
                  f"{'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)


def loop(case, n):
    import torch
    N = int(n)
    if case == "match":
        call, _, _ = prepared_match(N, *match_case(N, "blobs"), True)
    else:
        H, W, d = SHAPES[case]
        call, _, _ = prepared_labels(blobs(N, H, W), d)
    for _ in range(200): call()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"calls": calls, "loop": loop}[sys.argv[1]](*sys.argv[2:4])
