"""Developer aid (not collected by pytest): prints the byte layout the library carves -- camo_workspace_bytes, camo_batch_desc_bytes,
camo_shadow_bytes and camo_debug_ws_offset of every name -- over a grid of dims and batch shapes.  Needs no GPU.  A change that must
not move a buffer leaves this text as it was:

    python tools/dev/ws_layout_dump.py > before.txt     (on a build of the parent)
    python tools/dev/ws_layout_dump.py | diff before.txt -
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from camouflage_multimodal_amd import _lib

NAMES = ("R16 G16 Q16 Q2_16 KV16 KV2_16 O16 O2_16 Y16 Y2_16 XH16 XH2_16 rstd1 rstd2 mask1 mask2 lse2 X16 Wqkv_rg W1s W1T WcRgT "
         "dH16 dH2_16 dU16 dU2_16 dQKV16 dQKVkg16 dR16 dG16 dO2_16 delta2 dKV dQ2acc Ymean H1mean Y2mean H2mean "
         "R G Q KV2 KV Q2 P P2 O O2 U U2 Y Y2 H1 H2 comb fused F1 hid dhid dfused dF1 dcomb dHm1 dHm2").split()
# (rg_dim, kg_dim, hidden_dim, num_heads, num_classes, fusion_type)
DIMS = {"reference": (128, 128, 256, 8, 2, _lib.FUSION_CROSS_ATTENTION),
        "reference, 8 classes": (128, 128, 256, 8, 8, _lib.FUSION_CROSS_ATTENTION),
        "cross-attention 64/64/128, 4 heads": (64, 64, 128, 4, 2, _lib.FUSION_CROSS_ATTENTION),
        "late fusion, hidden 256": (128, 128, 256, 8, 2, _lib.FUSION_LATE)}
SHAPES = ((1, 1, 1), (1, 33, 13), (16, 7700, 13), (17, 7701, 16), (64, 30000, 13), (100, 47000, 13), (1024, 492000, 13))


def main():
    L = _lib.lib()
    assert len(NAMES) == 64
    for label, dims in DIMS.items():
        d = _lib.CamoDims(*dims, 0.3, None)
        print(f"== {label}: shadow_bytes {L.camo_shadow_bytes(C.byref(d))}")
        for B, T, Nk in SHAPES:
            print(f"-- B {B} T {T} Nk {Nk}: workspace_bytes {L.camo_workspace_bytes(C.byref(d), B, T, Nk)} desc_bytes {L.camo_batch_desc_bytes(B, T)}")
            for name in NAMES:
                print(f"{name} {L.camo_debug_ws_offset(C.byref(d), B, T, Nk, name.encode())}")


if __name__ == "__main__":
    main()
