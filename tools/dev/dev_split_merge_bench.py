"""Developer aid / measurement of the splitter's marker merging (include/camo_split_merge.h):
  python tools/dev/dev_split_merge_bench.py launches   microseconds per call of camo_split_merge at N = 16 of 256 x 256 and at one
                                                       1024 x 1024, on the parts camo_split_instances leaves at ratio 8/10 on
                                                       dev_split_bench.py's blob and noise label maps, at merge 4/5 and with the
                                                       prediction given; beside each time the split call's own on the same map, the
                                                       ratio to the call's traffic floor -- 4 B/pixel each of labels, parts and
                                                       prediction read, 4 B/pixel written, at the measured copy bandwidth -- and the
                                                       groups formed; `launches 16 blobs` runs one batch size and one content only
The library is called directly with every buffer allocated beforehand; the windows are dev_split_bench.py's (200 calls between two
device events, 50 at 1024 x 1024, the smallest of five windows and the largest beside it).  At 256 x 256 the outputs of every timed case
are checked against tests/split_merge_ref.py for the first image (at 1024 x 1024 the foreground and the id range).  No time is asserted."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_ref as M
from dev_instances_bench import COPY_BYTES_PER_US, SIZES, inputs
from dev_split_bench import ROWS, label_maps
from dev_timing import timed

RATIO, MERGE = (8, 10), (4, 5)


def launches(only_n=None, only_name=None):
    import torch
    from camouflage_multimodal_amd import _lib
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    for N, H, W, iters in SIZES:
        if only_n is not None and N != int(only_n): continue
        floor = N * H * W * 16 / COPY_BYTES_PER_US
        for name, pred in inputs(N, H, W).items():
            if only_name is not None and name != only_name: continue
            p, labels, min_area = label_maps(pred)
            dev = p.device
            st = _stream_ptr(dev)
            sbytes, mbytes = L.camo_split_workspace_bytes(N, H, W, 4), L.camo_split_merge_workspace_bytes(N, H, W)
            sws, mws = torch.empty(sbytes, dtype=torch.uint8, device=dev), torch.empty(mbytes, dtype=torch.uint8, device=dev)
            parts, out = torch.empty(N, H, W, dtype=torch.int32, device=dev), torch.empty(N, H, W, dtype=torch.int32, device=dev)
            table = torch.empty(N, ROWS, 8, dtype=torch.int64, device=dev)
            scounts, counts = torch.empty(N, 4, dtype=torch.int32, device=dev), torch.empty(N, 4, dtype=torch.int32, device=dev)

            def split():
                rc = L.camo_split_instances(_ptr(labels), _ptr(p), H * W, N, H, W, *RATIO, 0, 4, ROWS, _ptr(parts), _ptr(table), _ptr(scounts), _ptr(sws), sbytes, st)
                if rc != 0: raise RuntimeError(L.camo_last_error())

            def merge():
                rc = L.camo_split_merge(_ptr(labels), _ptr(parts), _ptr(p), H * W, N, H, W, *MERGE, ROWS, _ptr(out), _ptr(table), _ptr(counts), _ptr(mws), mbytes, st)
                if rc != 0: raise RuntimeError(L.camo_last_error())
            ts = timed(split, iters)
            t = timed(merge, iters)
            c = counts.cpu().numpy()
            if H * W <= 256 * 256:
                want = M.merge_image(labels[0].cpu().numpy(), parts[0].cpu().numpy(), pred[0], MERGE, ROWS)
                same = all(np.array_equal(a, b) for a, b in zip((out[0].cpu().numpy(), table[0].cpu().numpy(), c[0]), want[:3]))
                verdict = f"{'equal to' if same else 'DIFFERENT FROM'} the restatement"
            else:
                ok = bool(((out > 0) == (labels > 0)).all()) and int(out.max()) == int(c[:, 0].max())
                verdict = f"foreground and id range {'kept' if ok else 'WRONG'} (the restatement is not run at this size)"
            print(f"N = {N}, {H} x {W}, {name:5s} (min_area {min_area}): merge {t[0]:.1f} us (up to {t[1]:.1f}) per call = {t[0] / floor:.1f} x the traffic floor of "
                  f"{floor:.2f} us, {_lib.SPLIT_MERGE_LAUNCHES} launches; camo_split_instances on the same map {ts[0]:.1f} us (up to {ts[1]:.1f}); image 0: "
                  f"(K'', parts, groups of several, made whole) = {c[0].tolist()}; the batch: {c.sum(axis=0).tolist()}; {verdict}", flush=True)


if __name__ == "__main__":
    {"launches": launches}[sys.argv[1]](*sys.argv[2:4])
