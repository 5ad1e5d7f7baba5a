"""Developer aid / measurement of COCO run-length masks (include/camo_rle.h):
  python tools/dev/dev_rle_bench.py calls          at 256 x 256, N = 1 and N = 16, for the label maps mask_instances gives on blob and
                                                   on noise probability maps: microseconds per call of camo_rle_runs (R = 32768) and of
                                                   camo_rle_decode on the maps' own annotations, every buffer allocated beforehand; the
                                                   wall time of encode_instances (its default capacity of 4096 runs: the noise maps
                                                   take its second call) and decode_rles, host work and copies included; and
                                                   the host route they replace -- the label maps copied to the host and run through
                                                   the numpy restatement (tests/rle_ref.py), the decoded maps uploaded
  python tools/dev/dev_rle_bench.py loop 16 blobs  one batch size and one content only, 200 calls of each entry point (for a kernel trace)
A device window is 200 calls between two device events, the smallest of five windows is the figure and the largest is printed beside
it; a wall time is the smallest of three calls after a warm-up.  The outputs of every timed case are checked against the restatement.
No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rle_ref as R
from dev_timing import timed

H = W = 256
CAP = 32768


def inputs(N):
    """{"blobs", "noise"}: int32 [N, H, W] label maps on the device, from mask_instances."""
    import torch
    from camouflage_multimodal_amd import mask_instances
    rs = np.random.RandomState(N * 7 + 1)
    yy, xx = np.mgrid[:H, :W]
    blobs = np.zeros((N, H, W), np.float32)
    for i in range(N):
        for k in range(20):
            cy, cx, r = rs.randint(H // 8, H - H // 8), rs.randint(W // 8, W - W // 8), rs.randint(H // 32, H // 8)
            blobs[i][(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = rs.uniform(0.6, 1.0)
    noise = rs.uniform(0, 1, (N, H, W)).astype(np.float32)
    return {"blobs": mask_instances(torch.from_numpy(blobs).cuda(), 0.5, 8, 0, False, 64)["labels"],
            "noise": mask_instances(torch.from_numpy(noise).cuda(), 0.45, 8, 8, False, 64)["labels"]}


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


def prepared_runs(labels):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    N = labels.shape[0]
    nbytes = L.camo_rle_runs_workspace_bytes(N, H, W, CAP)
    runs, counts = torch.empty(N, CAP, 2, dtype=torch.int32, device=labels.device), torch.empty(N, 2, dtype=torch.int32, device=labels.device)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=labels.device)
    st = _stream_ptr(labels.device)

    def call():
        rc = L.camo_rle_runs(_ptr(labels), N, H, W, CAP, _ptr(runs), _ptr(counts), _ptr(ws), nbytes, st)
        if rc != 0: raise RuntimeError(L.camo_last_error())
    return call, runs, counts


def prepared_decode(rles):
    import torch
    from camouflage_multimodal_amd import _lib, rle as _rle
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    N = len(rles)
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
    return call, labels, (A, total)


def host_encode(labels):
    from camouflage_multimodal_amd import counts_to_string
    host = labels.cpu().numpy()
    return [{i: {"size": [H, W], "counts": counts_to_string(c)} for i, c in R.label_counts(l).items()} for l in host]


def host_decode(rles):
    import torch
    from camouflage_multimodal_amd import string_to_counts
    out = np.zeros((len(rles), H, W), np.int32)
    for n, image in enumerate(rles):
        for i, rle in image.items():
            out[n] = np.maximum(out[n], np.where(R.counts_mask(string_to_counts(rle["counts"]), H, W), i, 0))
    return torch.from_numpy(out).cuda()


def calls():
    import torch
    from camouflage_multimodal_amd import decode_rles, encode_instances
    for N in (1, 16):
        for name, labels in inputs(N).items():
            host = labels.cpu().numpy()
            call, runs, counts = prepared_runs(labels)
            t = timed(call, 200)
            want = R.runs_batch(host, CAP)
            same = np.array_equal(runs.cpu().numpy(), want["runs"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
            print(f"N = {N:2d}, {H} x {W}, {name:5s}: camo_rle_runs {t[0]:.1f} us (up to {t[1]:.1f}) per call, 3 launches; runs per image up to "
                  f"{int(want['counts'][:, 0].max())}, ids up to {int(host.max())}; {'equal to' if same else 'DIFFERENT FROM'} the restatement", flush=True)
            te, rles = wall(lambda: encode_instances(labels))
            th, ref = wall(lambda: host_encode(labels))
            print(f"        encode_instances {te:.0f} us wall; host route (copy of the maps, numpy runs per id, the strings) {th:.0f} us; "
                  f"{'equal' if rles == ref else 'DIFFERENT'}", flush=True)
            if not any(rles):
                continue
            call, back, (A, total) = prepared_decode(rles)
            t = timed(call, 200)
            same = torch.equal(back, labels)
            print(f"        camo_rle_decode {t[0]:.1f} us (up to {t[1]:.1f}) per call, 2 launches, {A} annotations, {total} counts; "
                  f"{'equal to' if same else 'DIFFERENT FROM'} the label maps", flush=True)
            td, dec = wall(lambda: decode_rles(rles, H, W))
            th, ref = wall(lambda: host_decode(rles))
            print(f"        decode_rles {td:.0f} us wall; host route (numpy paint per annotation, one upload) {th:.0f} us; "
                  f"{'equal' if torch.equal(dec, ref) and torch.equal(dec, labels) else 'DIFFERENT'}", flush=True)


def loop(n, name):
    import torch
    from camouflage_multimodal_amd import encode_instances
    labels = inputs(int(n))[name]
    call, _, _ = prepared_runs(labels)
    for _ in range(200): call()
    call, _, _ = prepared_decode(encode_instances(labels, CAP))
    for _ in range(200): call()
    torch.cuda.synchronize()


if __name__ == "__main__":
    {"calls": calls, "loop": loop}[sys.argv[1]](*sys.argv[2:4])
