"""Developer aid / measurement of the resize (include/camo_resize.h):
  python tools/dev/dev_resize_bench.py [out.json]
16 and 128 uint8 RGB images of mixed sizes around 1024 x 768 resized to 256 x 256, bilinear and area, and 128 fp32 maps of 256 x 256
resized back to those sizes, each three ways: the bare library call with the table already on the device (its time is the kernel's,
back to back), the Python surface (``resize_batch`` / ``resize_to_sizes``: table built, checked and uploaded per call, output
allocated), and the yardstick -- what a user does without it: one ``F.interpolate`` per image on the device and a ``torch.stack``.
Every case is warmed up; a window is as many calls as take at least a second between two device events; the versions alternate,
three windows each, the smallest is the figure and the largest is printed beside it.  Bytes = every source byte of the images once
plus every destination byte once, over the bare call's time.  No time is asserted."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZE = (256, 256)


def window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3                  # microseconds per call


def alternate(fns, windows=3):
    """{name: (least, most) microseconds per call}; the versions take turns, a window is at least a second."""
    import torch
    iters = {}
    for name, fn in fns.items():
        for _ in range(3): fn()
        torch.cuda.synchronize()
        iters[name] = max(3, int(1.1e6 / max(window(fn, 3), 1.0)))
    seen = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            seen[name].append(window(fn, iters[name]))
    return {name: (min(v), max(v)) for name, v in seen.items()}


def main():
    import torch
    import torch.nn.functional as F
    from camouflage_multimodal_amd import _lib, pack_images, resize_batch, resize_to_sizes
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    dev = torch.device("cuda")
    st = _stream_ptr(dev)
    rs = np.random.RandomState(0)
    results = []

    def report(case, n, bytes_moved, t):
        bare, surface, loop = t["bare call"], t["python surface"], t["torch loop"]
        row = {"case": case, "images": n, "bytes": bytes_moved, "bare_us": bare, "surface_us": surface, "torch_loop_us": loop,
               "bare_bytes_per_s": bytes_moved / (bare[0] * 1e-6), "loop_over_surface": loop[0] / surface[0]}
        results.append(row)
        print(f"{case:28s} N = {n:3d}: bare call {bare[0]:8.1f} us (up to {bare[1]:.1f}) = {row['bare_bytes_per_s'] / 1e9:7.1f} GB/s; "
              f"python surface {surface[0]:8.1f} us (up to {surface[1]:.1f}); torch loop {loop[0]:9.1f} us (up to {loop[1]:.1f}); "
              f"loop / surface = {row['loop_over_surface']:.2f}", flush=True)

    for n in (16, 128):
        sizes = [(int(rs.randint(600, 901)), int(rs.randint(800, 1201))) for _ in range(n)]
        images = [torch.from_numpy(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).to(dev) for h, w in sizes]
        packed = pack_images(images)
        Ho, Wo = SIZE
        rows = [[o, h, w, w * 3, 3, 1, 0, 0, h, w, 0, i * Ho * Wo * 3, Ho, Wo, Wo * 3, 3, 1, 0] for i, (o, (h, w)) in enumerate(zip(packed.offsets(), sizes))]
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        out = torch.empty(n, Ho, Wo, 3, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        moved = packed.data.numel() + out.numel() * 4
        for name in ("bilinear", "area"):
            code = {"bilinear": _lib.RSZ_BILINEAR, "area": _lib.RSZ_AREA}[name]

            def bare():
                rc = L.camo_resize(_ptr(packed.data), packed.data.numel(), _lib.RSZ_U8, _ptr(out), out.numel(), _lib.RSZ_F32, _ptr(table), n, 3, code,
                                   Ho * Wo, _ptr(status), st)
                if rc != 0: raise RuntimeError(L.camo_last_error())

            def loop():
                return torch.stack([F.interpolate(im.permute(2, 0, 1).unsqueeze(0).float(), size=SIZE, mode=name,
                                                  **({"align_corners": False} if name == "bilinear" else {}))[0].permute(1, 2, 0) for im in images]) / 255
            got, want = resize_batch(packed, SIZE, name), loop()
            print(f"  ({name}: largest difference from the torch loop {float((got - want).abs().max()):.3g})", flush=True)
            report(f"u8 -> {Ho} x {Wo} fp32, {name}", n, moved, alternate({"bare call": bare, "python surface": lambda: resize_batch(packed, SIZE, name), "torch loop": loop}))
        if n == 128:
            maps = torch.rand(n, 3, Ho, Wo, device=dev)
            rows, at = [], 0
            for i, (h, w) in enumerate(sizes):
                rows.append([i * 3 * Ho * Wo, Ho, Wo, Wo, 1, Ho * Wo, 0, 0, Ho, Wo, 0, at, h, w, w, 1, h * w, 0])
                at += h * w
            table = torch.tensor(rows, dtype=torch.int64).to(dev)
            big = torch.empty(at, device=dev)
            mdp = max(h * w for h, w in sizes)

            def bare_up():
                rc = L.camo_resize(_ptr(maps), maps.numel(), _lib.RSZ_F32, _ptr(big), at, _lib.RSZ_F32, _ptr(table), n, 1, _lib.RSZ_BILINEAR, mdp, _ptr(status), st)
                if rc != 0: raise RuntimeError(L.camo_last_error())

            def loop_up():
                return [F.interpolate(maps[i:i + 1, 0:1], size=sizes[i], mode="bilinear", align_corners=False)[0, 0] for i in range(n)]
            views, _ = resize_to_sizes(maps[:, 0], sizes)
            print(f"  (maps up: largest difference from the torch loop {max(float((a - b).abs().max()) for a, b in zip(views, loop_up())):.3g})", flush=True)
            report(f"fp32 {Ho} x {Wo} -> native, bilinear", n, n * Ho * Wo * 4 + at * 4,
                   alternate({"bare call": bare_up, "python surface": lambda: resize_to_sizes(maps[:, 0], sizes), "torch loop": loop_up}))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
