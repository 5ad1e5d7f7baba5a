"""Builds the HIP shared library in-tree (gfx950 only).

    python -m camouflage_multimodal_amd.build [--force]

hipcc cross-compiles without a GPU, so this runs in the build container; the
resulting ``libcamo_fusion.so`` sits next to this file and travels to the GPU box
with the repository snapshot (it is git-ignored, not gpurun-ignored).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcamo_fusion.so")
SOURCES = ("gemm.hip", "gemm16.hip", "attn.hip", "attn_fast.hip", "attn_mfma.hip", "misc.hip", "rg_gnn.hip", "rg_features.hip", "rg_batch.hip", "fused_rows.hip", "fused_wide.hip", "fused_wide2.hip", "bwd_wide2.hip", "tail_wide.hip", "attn_maps.hip", "fusion_abi.hip", "rg_abi.hip", "image_abi.hip", "canny.hip", "slic.hip", "rg_detect.hip", "rg_train.hip", "rg_targets.hip", "rg_pixel_loss.hip", "seg_measures.hip", "resize.hip", "instances.hip", "inst_match.hip", "boundary.hip", "guided.hip", "rle.hip", "poly.hip", "contours.hip", "split.hip", "split_geo.hip", "split_merge.hip", "augment.hip")
HEADERS = ("common.h", "abi_util.h", "fusion_ws.h", "gemm.h", "gemm16.h", "attn.h", "misc.h", "rg_gnn.h", "rg_features.h", "rg_batch.h", "canny.h", "slic.h", "rg_detect.h", "rg_train.h", "rg_targets.h", "rg_pixel_loss.h", "seg_measures.h", "instances.h", "inst_match.h", "boundary.h", "guided.h", "rle.h", "poly.h", "contours.h", "split.h", "split_inl.h", "inst_emit_inl.h", "resize_taps.h", "cc_inl.h", "label_inl.h", "fused_rows.h", "shadow_inl.h", "mfma_inl.h", "wide2_inl.h", "tail_wide.h", "attn_maps.h", os.path.join("..", "..", "include", "camo_fusion.h"), os.path.join("..", "..", "include", "camo_rg_gnn.h"), os.path.join("..", "..", "include", "camo_rg_features.h"), os.path.join("..", "..", "include", "camo_rg_batch.h"), os.path.join("..", "..", "include", "camo_canny.h"), os.path.join("..", "..", "include", "camo_slic.h"), os.path.join("..", "..", "include", "camo_rg_detect.h"), os.path.join("..", "..", "include", "camo_rg_train.h"), os.path.join("..", "..", "include", "camo_rg_train_bn.h"), os.path.join("..", "..", "include", "camo_rg_train_drop.h"), os.path.join("..", "..", "include", "camo_rg_targets.h"), os.path.join("..", "..", "include", "camo_rg_pixel_loss.h"), os.path.join("..", "..", "include", "camo_seg_measures.h"), os.path.join("..", "..", "include", "camo_resize.h"), os.path.join("..", "..", "include", "camo_instances.h"), os.path.join("..", "..", "include", "camo_inst_match.h"), os.path.join("..", "..", "include", "camo_boundary.h"), os.path.join("..", "..", "include", "camo_guided.h"), os.path.join("..", "..", "include", "camo_rle.h"), os.path.join("..", "..", "include", "camo_poly.h"), os.path.join("..", "..", "include", "camo_contours.h"), os.path.join("..", "..", "include", "camo_split.h"), os.path.join("..", "..", "include", "camo_split_geo.h"), os.path.join("..", "..", "include", "camo_split_merge.h"), os.path.join("..", "..", "include", "camo_augment.h"))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# per-file additions.  fused_wide2.hip: no SLP vectorisation (v_pk_*_f32 beside MFMAs cost more issue time than the two scalar
# instructions they replace: MI355X guide, cycle constants) and no NaN canonicalisation in front of every v_max_f32 (the kernel
# compares finite scores; a NaN input still comes out as a NaN through the sums)
# poly.hip: include/camo_poly.h rounds every product and sum once, so no contraction into fused multiply-adds
EXTRA_FLAGS = {"fused_wide2.hip": ["-fno-slp-vectorize", "-fno-honor-nans"], "bwd_wide2.hip": ["-fno-slp-vectorize", "-fno-honor-nans"],
               "poly.hip": ["-ffp-contract=off"]}


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (looked at $HIPCC, /opt/rocm/bin/hipcc, PATH)")


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not _stale():
        return LIB
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src):
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = [hipcc, *FLAGS, *EXTRA_FLAGS.get(src, []), "-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            sys.stderr.write(r.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"built {LIB}")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
