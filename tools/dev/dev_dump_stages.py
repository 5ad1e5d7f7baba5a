"""Developer aid: dump every saved / staged tensor of one training call of the fused row-tile schedule, or compare two dumps.
   python tools/dev/dev_dump_stages.py dump OUT.npz        (bench.py's batch 0 and a ragged batch, dropout 0.3, fixed seeds)
   python tools/dev/dev_dump_stages.py compare A.npz B.npz (A, B: dumps of two builds of the library)
The tensors are read from the call's private workspace through the debug offsets the stage tests use (camo_debug_ws_offset).  The
comparison is bit for bit for every tensor no float atomic feeds; the atomics' sums (Ymean, Hmean, dQ2acc, dKV when it is not summed
through slabs, the gradients) and what is computed from them are held to the stage test's relative bound instead."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H = 256
# name -> (rows: "T" RG rows / "K" KG rows / "B" per sample / "1", columns, bytes per element)
EXACT = {"X16": ("T", 128, 2), "R16": ("T", H, 2), "G16": ("K", H, 2), "Q16": ("T", H, 2), "Q2_16": ("K", H, 2), "KV16": ("K", 2 * H, 2),
         "KV2_16": ("T", 2 * H, 2), "O16": ("T", H, 2), "O2_16": ("K", H, 2), "Y16": ("T", H, 2), "Y2_16": ("K", H, 2), "XH16": ("T", H, 2),
         "XH2_16": ("K", H, 2), "rstd1": ("T", 1, 4), "rstd2": ("K", 1, 4), "lse2": ("B", 8 * 16 * 2, 4), "mask1": ("T", 16, 4), "mask2": ("K", 16, 4),
         "dU16": ("T", H, 2), "dU2_16": ("K", H, 2), "dO2_16": ("K", H, 2), "delta2": ("B", 8 * 16, 4), "dQKV16": ("T", 3 * H, 2), "dR16": ("T", H, 2),
         "dH16": ("T", 2 * H, 2), "dH2_16": ("K", 2 * H, 2)}
# behind float atomics (or computed from their sums): compared with a tolerance
CLOSE = {"Ymean": ("B", H, 4), "Y2mean": ("B", H, 4), "H1mean": ("B", 2 * H, 4), "H2mean": ("B", 2 * H, 4), "dQ2acc": ("K", H, 4), "dKV": ("K", 2 * H, 4),
         "dQKVkg16": ("K", 3 * H, 2)}
RAGGED = [1, 31, 32, 33, 65, 303, 127]


def dump(out):
    import torch
    from bench import make_batches
    from camouflage_multimodal_amd import _lib, build_multimodal_model
    L = _lib.lib()
    res = {}
    rgb, nrsb, kgb, *_ = make_batches(1, 16, 0)[0]
    rng = np.random.default_rng(5)
    cases = {"bench0": (rgb, list(nrsb), kgb),
             "ragged": (rng.standard_normal((sum(RAGGED), rgb.shape[1])).astype(np.float32), RAGGED,
                        rng.standard_normal((len(RAGGED),) + kgb.shape[1:]).astype(np.float32))}
    for cname, (rg, nrs, kg) in cases.items():
        torch.manual_seed(0)
        m = build_multimodal_model({"dropout": 0.3}).cuda().set_precision("bf16").train()
        eng = m._engine
        batch = eng.make_batch(torch.from_numpy(rg).cuda(), nrs, torch.from_numpy(kg).cuda())
        ws = eng.workspace(batch, private=True)
        ws.zero_()
        g = eng.ensure_flat_grads(attach=True)
        g.zero_()
        seed = 0x1234ABCD5678
        outs, _ = eng.forward_raw(batch, ws, True, seed)
        flat = lambda o: o.float() if torch.is_tensor(o) else torch.cat([x.reshape(batch.B, -1).float() for x in o], dim=1)
        d_outs = (flat(outs) * 0.01 + 0.001).contiguous()
        eng.backward_raw(batch, ws, outs, d_outs, True, seed, eng._gtab)
        torch.cuda.synchronize()
        rows = {"T": batch.T, "K": batch.B * batch.Nk, "B": batch.B, "1": 1}
        for name, (r, cols, eb) in {**EXACT, **CLOSE}.items():
            off = L.camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
            if off < 0:
                continue
            n = rows[r] * cols * eb
            res[f"{cname}/{name}"] = ws[off:off + n].cpu().numpy().copy().view(np.uint16 if eb == 2 else np.uint32)
        # the slabs: this call's rows only (one row of 512 per tile and KG block; Nk rows of 512 per tile)
        tiles = sum((n + 31) // 32 for n in nrs)
        for name, n in (("slabLN", (tiles + batch.B) * 512), ("slabKV", tiles * batch.Nk * 512)):
            off = L.camo_debug_ws_offset(C.byref(eng.dims), batch.B, batch.T, batch.Nk, name.encode())
            if off >= 0:
                res[f"{cname}/{name}"] = ws[off:off + 4 * n].cpu().numpy().copy().view(np.uint32)
        res[f"{cname}/outs"] = flat(outs).cpu().numpy().view(np.uint32)
        res[f"{cname}/~grads"] = g.cpu().numpy().copy()
    np.savez(out, **res)
    print(f"dumped {len(res)} arrays to {out}")


def as_f32(name, a):
    return (a.astype(np.uint32) << 16).view(np.float32) if a.dtype == np.uint16 else a.view(np.float32)


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    assert sorted(A.files) == sorted(B.files), (sorted(set(A.files) ^ set(B.files)))
    bad = n_exact = n_close = 0
    for k in sorted(A.files):
        base = k.split("/")[1]
        a, b = A[k], B[k]
        if base in CLOSE or base == "~grads":
            # the stage test's bound for sums of atomics: |err| <= 5e-2 * max|want| on all but 2 % of the elements, mean <= 1e-2
            fa, fb = (a, b) if base == "~grads" else (as_f32(k, a), as_f32(k, b))
            fa, fb = fa.astype(np.float64), fb.astype(np.float64)
            scale = max(np.abs(fa).max(), 1e-6)
            err = np.abs(fa - fb)
            ok = (err > 5e-2 * scale).mean() <= 2e-2 and err.mean() <= 1e-2 * scale and np.isfinite(fb).all()
            n_close += 1
            print(f"{'ok  ' if ok else 'FAIL'} close  {k:24s} max |diff| / scale {err.max() / scale:.2e}  bitwise equal: {np.array_equal(a, b)}")
            if not ok:
                print("     largest differences at flat indices", np.argsort(-err.reshape(-1))[:8].tolist())
        else:
            ok = np.array_equal(a, b)
            n_exact += 1
            if not ok:
                d = np.nonzero(a != b)[0]
                print(f"FAIL exact  {k:24s} {len(d)} of {a.size} elements differ, first at {d[0]}")
        bad += not ok
    print(f"{n_exact} arrays compared bit for bit, {n_close} with the atomics' tolerance: {'all agree' if not bad else str(bad) + ' DIFFER'}")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
