"""Developer aid / measurement of the training augmentation (include/camo_augment.h):
  python tools/dev/dev_augment_bench.py launches   microseconds per call of camo_augment against camo_resize bilinear on the SAME batch in
                                                   the same session: 16 images of 768 x 1024 -> 256 x 256 and 16 of 256 x 256 -> 256 x 256,
                                                   uint8 RGB to fp32; camo_resize with a crop and a flip per image, camo_augment with the
                                                   same crops and flips stated as maps (warp only: the same bytes are checked), with a
                                                   rotation per image (warp only), and with the rotation and the four enhancements; the
                                                   four calls alternate window by window
  python tools/dev/dev_augment_bench.py step       milliseconds per RegionGraphFineTuner.step_from_ragged on 16 images of 256 x 256 ->
                                                   256 x 256, 500 superpixels: with crops and flips, with augment= stating the same crops
                                                   and flips (no turn, no factors: what the keyword itself costs) and with a drawn
                                                   augment= (whose images segment differently: the node counts are printed), alternating
  python tools/dev/dev_augment_bench.py host       the numpy restatement of one 256 x 256 image on one host core (needs no GPU)
The library is called directly with every buffer allocated beforehand; every case is warmed up; a window is 200 calls between two
device events, the smallest of five windows is the figure and the largest is printed beside it.  The first image of every timed
camo_augment case is checked against the restatement.  No time is asserted."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as AR
from dev_timing import alternate

SIZE = (256, 256)
BATCHES = ((16, 768, 1024), (16, 256, 256))


def scene(N, H, W, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(N)]


def launches():
    import torch
    from camouflage_multimodal_amd import _lib, pack_images, random_resized_crops
    from camouflage_multimodal_amd.augment import affine_rows, random_cod_augmentation
    from camouflage_multimodal_amd.engine import _ptr, _stream_ptr
    L = _lib.lib()
    Ho, Wo = SIZE
    for N, H, W in BATCHES:
        images = scene(N, H, W)
        packed = pack_images(images)
        dev = packed.data.device
        st = _stream_ptr(dev)
        sizes = [(H, W)] * N
        crops, flips = random_resized_crops(sizes, seed=1)
        aug = random_cod_augmentation(sizes, SIZE, seed=1, rotate_p=1.0)
        geo = [[o, H, W, 3 * W, 3, 1] for o in packed.offsets()]
        rtable = torch.tensor([g + list(c) + [f, i * Ho * Wo * 3, Ho, Wo, Wo * 3, 3, 1, 0] for i, (g, c, f) in enumerate(zip(geo, crops, flips))],
                              dtype=torch.int64).to(dev)
        same = affine_rows(sizes, SIZE, crops, flips, border="replicate")
        turned = affine_rows(sizes, SIZE, aug["crops"], aug["flips"], aug["angles"])
        tables = {"same": [g + r + [0] * 6 for g, r in zip(geo, same)], "turned": [g + r + [0] * 6 for g, r in zip(geo, turned)],
                  "enhanced": [g + r + list(k) + [0, 0] for g, r, k in zip(geo, turned, aug["factors"])]}
        dtab = {k: torch.tensor(v, dtype=torch.int64).to(dev) for k, v in tables.items()}
        out = {k: torch.empty(N, Ho, Wo, 3, device=dev) for k in ("resize", *tables)}
        status = torch.empty(N, dtype=torch.int32, device=dev)
        nbytes = int(L.camo_augment_workspace_bytes(N, Ho, Wo, 3, 1))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        elems = packed.data.numel()

        def resize():
            rc = L.camo_resize(_ptr(packed.data), elems, _lib.RSZ_U8, _ptr(out["resize"]), N * Ho * Wo * 3, _lib.RSZ_F32, _ptr(rtable), N, 3,
                               _lib.RSZ_BILINEAR, Ho * Wo, _ptr(status), st)
            if rc != 0: raise RuntimeError(L.camo_last_error())

        def augment(name):
            def call():
                rc = L.camo_augment(_ptr(packed.data), elems, _ptr(out[name]), _lib.RSZ_F32, _ptr(dtab[name]), N, 3, Ho, Wo, _lib.RSZ_BILINEAR,
                                    int(name == "enhanced"), _ptr(status), _ptr(ws), nbytes, st)
                if rc != 0: raise RuntimeError(L.camo_last_error())
            return call
        t = alternate({"resize": resize, **{k: augment(k) for k in tables}}, 200)
        equal = bool(torch.equal(out["resize"], out["same"]))
        checks = []
        for name in tables:
            want, wstatus = AR.run_table(packed.data[:H * W * 3].cpu().numpy(), np.array(tables[name][:1], np.int64), 3, SIZE, "bilinear", name == "enhanced", "f32")
            checks.append(f"{name} {'equal to' if np.array_equal(out[name][0].cpu().numpy(), want[0]) else 'DIFFERENT FROM'} the restatement")
        floor_note = f"bytes written {N * Ho * Wo * 12}"
        print(f"N = {N}, {H} x {W} -> {Ho} x {Wo}, u8 RGB -> fp32 ({floor_note}): camo_resize bilinear {t['resize'][0]:.1f} us (up to {t['resize'][1]:.1f}); "
              f"camo_augment the same crops and flips {t['same'][0]:.1f} us (up to {t['same'][1]:.1f}), bytes {'equal' if equal else 'DIFFERENT'}; "
              f"turned, warp only {t['turned'][0]:.1f} us (up to {t['turned'][1]:.1f}); turned and enhanced (3 launches) {t['enhanced'][0]:.1f} us "
              f"(up to {t['enhanced'][1]:.1f}); image 0: {', '.join(checks)}", flush=True)


def step():
    import torch
    from camouflage_multimodal_amd import RegionGraphFineTuner, RegionGraphGNN, pack_images, prepare_finetune_batch_ragged, random_resized_crops
    from camouflage_multimodal_amd.augment import random_cod_augmentation
    N, H, W = BATCHES[1]
    images = scene(N, H, W)
    yy, xx = np.mgrid[:H, :W]
    masks = [np.where((yy - H * 0.4) ** 2 + (xx - W * 0.55) ** 2 < (H * 0.3) ** 2, 255, 0).astype(np.uint8)] * N
    packed, pmasks = pack_images(images), pack_images(masks)
    sizes = [(H, W)] * N
    crops, flips = random_resized_crops(sizes, seed=1)
    aug = random_cod_augmentation(sizes, SIZE, seed=1)
    torch.manual_seed(0)
    tuner = RegionGraphFineTuner(RegionGraphGNN().cuda(), lr=1e-4, seed=0)

    same = {"crops": crops, "flips": flips, "angles": [0.0] * N, "factors": None}      # the plain call's images but for the border rule
    cases = {"plain": dict(crops=crops, flips=flips), "same": dict(augment=same), "augmented": dict(augment=aug)}
    nodes = {k: int(prepare_finetune_batch_ragged(packed, pmasks, size=SIZE, device=packed.data.device, **kw).graphs.x.shape[0]) for k, kw in cases.items()}
    t = alternate({k: (lambda kw=kw: tuner.step_from_ragged(packed, pmasks, size=SIZE, **kw)) for k, kw in cases.items()}, 20)
    print(f"step_from_ragged, N = {N}, {H} x {W} -> {SIZE[0]} x {SIZE[1]}, 500 superpixels (preparation and step, host included): crops and flips "
          f"{t['plain'][0] / 1e3:.2f} ms (up to {t['plain'][1] / 1e3:.2f}), {nodes['plain']} nodes; augment= with the same crops and flips, no turn, no factors "
          f"{t['same'][0] / 1e3:.2f} ms (up to {t['same'][1] / 1e3:.2f}), {nodes['same']} nodes; augment= drawn (turn and four factors) "
          f"{t['augmented'][0] / 1e3:.2f} ms (up to {t['augmented'][1] / 1e3:.2f}), {nodes['augmented']} nodes", flush=True)


def host():
    from camouflage_multimodal_amd.augment import affine_rows
    img = scene(1, 256, 256)[0]
    r = affine_rows([(256, 256)], SIZE, angles=[10.0])[0]
    t0 = time.perf_counter()
    AR.enhance(AR.warp(img, SIZE, r[:4], r[4:10], r[10], r[11], "bilinear", "u8"), (300, 200, 400, 500))
    print(f"numpy restatement, one 256 x 256 image, warp and enhancements: {(time.perf_counter() - t0) * 1e3:.0f} ms (one host core)", flush=True)


if __name__ == "__main__":
    {"launches": launches, "step": step, "host": host}[sys.argv[1]]()
