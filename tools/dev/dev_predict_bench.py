"""Developer aid: the prediction API in bf16 mode.
   python tools/dev/dev_predict_bench.py                 wall clock per image of 256 predictions through predict_embedding_directory at
                                                         batch_size 1 / 16 / 256 (final synchronise; batch_size = 1 is the per-image loop), and of
                                                         predict_batch_from_embeddings with its attention maps at 16 / 256 images per call
   python tools/dev/dev_predict_bench.py kernel B [n]    n (default 50) maps calls of B images and n plain inference calls, nothing else: run it under
                                                         rocprofv3 --kernel-trace --stats (a run of its own) for attn_maps_kernel's time next to the
                                                         forward's launches; prints the bytes the maps kernel must move per call"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from camouflage_multimodal_amd import (build_multimodal_model, predict_batch_from_embeddings,  # noqa: E402
                                       predict_embedding_directory)

HIST = [303, 481, 500, 530, 441, 447, 512, 388]
torch.manual_seed(0)
model = build_multimodal_model({}).cuda().set_precision("bf16").eval()
rs = np.random.RandomState(0)
kg = {f"cat_{i:02d}": torch.from_numpy(np.abs(rs.standard_normal((1, 128))).astype(np.float32) * 0.3) for i in range(13)}


def images(n):
    return {f"img_{i:04d}": {"node_embeddings": torch.from_numpy(np.abs(rs.standard_normal((HIST[i % len(HIST)], 128))).astype(np.float32) * 0.3)}
            for i in range(n)}


if len(sys.argv) > 1 and sys.argv[1] == "kernel":
    B, n = int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 50
    imgs = [v["node_embeddings"].cuda() for v in images(B).values()]
    nrs = [int(r.shape[0]) for r in imgs]
    rg, kgt = torch.cat(imgs), torch.stack([v.reshape(-1) for v in kg.values()]).cuda()[None].expand(B, -1, -1).contiguous()
    with torch.no_grad():
        for attention in (True, False):
            for _ in range(n):
                model.forward_packed(rg, nrs, kgt, return_attention=attention, fused_attention=True)
    torch.cuda.synchronize()
    T, Nk = sum(nrs), 13
    rd, wr = T * (512 + 512) + len(nrs) * (Nk * (1024 + 512) + 8 * 16 * 8), 2 * T * Nk * 4
    print(f"B={B} T={T}: attn_maps_kernel reads {rd} B (Q16 row + K half of the KV2_16 row per RG row; the sample's KV16 / Q2_16 rows, lse2) and writes {wr} B "
          f"per call = {(rd + wr) / 1e6:.3f} MB; {n} maps calls then {n} plain calls")
    sys.exit(0)

N = 256
imgs = images(N)
out = tempfile.mkdtemp()
for bs in (1, 16, 256):
    predict_embedding_directory(model, imgs, kg, out, "cuda", max_images=2 * bs, batch_size=bs)       # warm-up (weight shadows, descriptors, workspace)
    torch.cuda.synchronize()
    best = 1e9
    for rep in range(3):
        t0 = time.perf_counter()
        predict_embedding_directory(model, imgs, kg, out, "cuda", batch_size=bs)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    print(f"predict_embedding_directory batch_size={bs:3d}: {best / N * 1e6:9.1f} us/image (best of 3 runs over {N} images, JSON write included)")
lst = [v["node_embeddings"] for v in imgs.values()]
for bs in (16, 256):
    predict_batch_from_embeddings(model, lst[:bs], kg, "cuda")
    torch.cuda.synchronize()
    best = 1e9
    for rep in range(3):
        t0 = time.perf_counter()
        for g in range(0, N, bs):
            predict_batch_from_embeddings(model, lst[g:g + bs], kg, "cuda")
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    print(f"predict_batch_from_embeddings with maps, {bs:3d} images per call: {best / N * 1e6:9.1f} us/image")
