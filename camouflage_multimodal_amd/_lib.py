"""ctypes binding of the headers under include/.

There is no CPU fallback: if the shared library is missing or the tensors are
not on a HIP device the callers raise.  Build with
``python -m camouflage_multimodal_amd.build`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcamo_fusion.so")

ABI_VERSION = 13
FWD_INFERENCE = 1
FLAG_ATTN_MAPS = 2
FWD_FUSED_MAPS = 4
SUMSQ_FLOATS = 257
FUSION_CROSS_ATTENTION, FUSION_LATE = 0, 1
PREC_F32, PREC_BF16 = 0, 1
NPARAMS_CROSS, NPARAMS_LATE = 44, 22

RGB_TILE_SLOTS = 64                 # CAMO_RGB_TILE_SLOTS
RGB_VAR_BOUND = 3.0 * 2.0 ** -37    # CAMO_RGB_VAR_BOUND
RG_VAR_BOUND_PER_PIXEL = 9.0 * 2.0 ** -53      # CAMO_RG_VAR_BOUND_PER_PIXEL: times a region's pixels, camo_rg_region_graph's variances
RGD_NPARAMS = 12                    # CAMO_RGD_NPARAMS
RGD_MAX_CHANNELS = 16               # CAMO_RGD_MAX_CHANNELS
RGD_FIX_BITS = 32                   # CAMO_RGD_FIX_BITS
RGT_NGRADS = 32                     # CAMO_RGT_NGRADS
RGPL_MAX_RADIUS = 31                # CAMO_RGPL_MAX_RADIUS
RGPL_MAX_GAIN = 16                  # CAMO_RGPL_MAX_GAIN
SEG_BINS = 256                      # CAMO_SEG_BINS
SEG_QUADRANTS = 4                   # CAMO_SEG_QUADRANTS
SEG_HIST_INTS = 2048                # CAMO_SEG_HIST_INTS
SEG_WF_MAX_SIDE = 2048              # CAMO_SEG_WF_MAX_SIDE
RGD_MAX_IMAGES = 65535              # CAMO_RGD_MAX_IMAGES
RSZ_FIELDS = 18                     # CAMO_RSZ_FIELDS
RSZ_MAX_SIDE = 8192                 # CAMO_RSZ_MAX_SIDE
RSZ_MAX_CHANNELS = 4                # CAMO_RSZ_MAX_CHANNELS
RSZ_NEAREST, RSZ_BILINEAR, RSZ_AREA = 0, 1, 2      # CAMO_RSZ_NEAREST, CAMO_RSZ_BILINEAR, CAMO_RSZ_AREA
RSZ_U8, RSZ_F32 = 0, 1              # CAMO_RSZ_U8, CAMO_RSZ_F32
AUG_FIELDS = 24                     # CAMO_AUG_FIELDS
AUG_FRAC_BITS = 16                  # CAMO_AUG_FRAC_BITS
AUG_MAX_FACTOR = 1024               # CAMO_AUG_MAX_FACTOR
AUG_TILE = 32                       # CAMO_AUG_TILE
INST_FIELDS = 8                     # CAMO_INST_FIELDS
INST_COUNTS = 4                     # CAMO_INST_COUNTS
INST_MAX_ROWS = 1 << 24             # CAMO_INST_MAX_ROWS
IM_MAX_THRESHOLDS = 16              # CAMO_IM_MAX_THRESHOLDS
IM_MAX_IDS = 1024                   # CAMO_IM_MAX_IDS
IM_MAX_CELLS = 1 << 26              # CAMO_IM_MAX_CELLS
IM_COUNTS = 4                       # CAMO_IM_COUNTS
BD_MAX_DISTANCE = 1 << 12           # CAMO_BD_MAX_DISTANCE
BD_STRIP = 64                       # CAMO_BD_STRIP
BD_ROW_FIELDS = 6                   # CAMO_BD_ROW_FIELDS
BD_GT_FIELDS = 2                    # CAMO_BD_GT_FIELDS
RLE_MAX_ROWS = 1 << 26              # CAMO_RLE_MAX_ROWS
RLE_MAX_ANNOTATIONS = 65535         # CAMO_RLE_MAX_ANNOTATIONS
RLE_MAX_COUNTS = 1 << 26            # CAMO_RLE_MAX_COUNTS
POLY_MAX_ANNOTATIONS = 65535        # CAMO_POLY_MAX_ANNOTATIONS
POLY_MAX_POLYGONS = 65535           # CAMO_POLY_MAX_POLYGONS
POLY_MAX_VERTICES = 1 << 20         # CAMO_POLY_MAX_VERTICES
POLY_MARGIN = 1024                  # CAMO_POLY_MARGIN
POLY_MAX_PLANE_WORDS = 1 << 28      # CAMO_POLY_MAX_PLANE_WORDS
CONTOUR_RING_FIELDS = 5             # CAMO_CONTOUR_RING_FIELDS
CONTOUR_COUNTS = 6                  # CAMO_CONTOUR_COUNTS
CONTOUR_MAX_CRACKS = 1 << 26        # CAMO_CONTOUR_MAX_CRACKS
CONTOUR_MAX_RINGS = 1 << 24         # CAMO_CONTOUR_MAX_RINGS
CONTOUR_MAX_VERTICES = 1 << 26      # CAMO_CONTOUR_MAX_VERTICES
CONTOUR_LDS_CRACKS = 1 << 14        # CAMO_CONTOUR_LDS_CRACKS
SPLIT_MAX_SPLIT = 8                 # CAMO_SPLIT_MAX_SPLIT
SPLIT_MAX_DEN = 16                  # CAMO_SPLIT_MAX_DEN
SPLIT_COUNTS = 4                    # CAMO_SPLIT_COUNTS
SPLIT_LAUNCHES = 13                 # CAMO_SPLIT_LAUNCHES
SPLIT_GEO_TILE = 32                 # CAMO_SPLIT_GEO_TILE
SPLIT_GEO_MAX_ROUNDS = 1024         # CAMO_SPLIT_GEO_MAX_ROUNDS
SPLIT_GEO_LAUNCHES = 13             # CAMO_SPLIT_GEO_LAUNCHES (plus the rounds)
SPLIT_GEO_RESUME_LAUNCHES = 2       # CAMO_SPLIT_GEO_RESUME_LAUNCHES (plus the rounds)
SPLIT_MERGE_COUNTS = 4              # CAMO_SPLIT_MERGE_COUNTS
SPLIT_MERGE_LAUNCHES = 6            # CAMO_SPLIT_MERGE_LAUNCHES
GF_MAX_RADIUS = 64                  # CAMO_GF_MAX_RADIUS
GF_MIN_EPS, GF_MAX_EPS = 1e-6, 1.0  # CAMO_GF_MIN_EPS, CAMO_GF_MAX_EPS
GF_FIELDS = 4                       # CAMO_GF_FIELDS
RG_MAX_LABELS = 4096
RG_NPARAMS = 28


class CamoRgDims(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32)]


OPTION_NAMES = ("sched16", "fused", "tail17", "fused_rt", "wide2", "fused_one", "wide_front_rt", "tailw", "tailw_bwd", "param_space", "tn_big",
                "fused_variant", "back_lead", "tn_balance", "tn_kcap", "tn_exp", "exp", "fused_save", "tail_skip_arrival", "wide2_bwd")


class CamoOptions(C.Structure):
    """camo_options_t (include/camo_fusion.h): the schedule options of ONE engine -- caller-owned, reached through CamoDims.options."""
    _fields_ = [(n, C.c_int32) for n in OPTION_NAMES]


# camo_options_init's values (a CPU test holds the two to each other): an engine can be constructed before the library is loadable
OPTION_DEFAULTS = dict(sched16=-1, fused=-1, tail17=-1, fused_rt=-1, wide2=-1, fused_one=1, wide_front_rt=0, tailw=-1, tailw_bwd=-1, param_space=-1, tn_big=-1,
                       fused_variant=1, back_lead=1, tn_balance=1, tn_kcap=0, tn_exp=0, exp=0, fused_save=0, tail_skip_arrival=0, wide2_bwd=-1)


def default_options():
    o = CamoOptions()
    for k, v in OPTION_DEFAULTS.items():
        setattr(o, k, v)
    return o


class CamoDims(C.Structure):
    _fields_ = [("rg_dim", C.c_int32), ("kg_dim", C.c_int32), ("hidden_dim", C.c_int32), ("num_heads", C.c_int32),
                ("num_classes", C.c_int32), ("fusion_type", C.c_int32), ("dropout", C.c_float), ("options", C.POINTER(CamoOptions))]


CALL_FORWARD, CALL_BACKWARD, CALL_TRAIN = 0, 1, 2
PLAN_FIELDS = ("nodes", "shadows", "save", "front", "front_rt", "back", "back_rt", "save_r16", "tail", "tail_wg", "loss", "tail_event", "param_space", "bwd1", "bwd2", "maps")


class CamoPlan(C.Structure):
    """camo_plan_t (include/camo_fusion.h): the launch schedule of one call, as camo_debug_plan reports it."""
    _fields_ = [(n, C.c_int32) for n in PLAN_FIELDS]


vp, i32, i64, u64, f32, f64, sz, P = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_size_t, C.POINTER
dims, rgdims = P(CamoDims), P(CamoRgDims)

# THE restatement of include/*.h: header -> (name, restype, argtypes) of every function it declares, in the header's order.
# lib() binds from it and tests/test_abi_binding.py holds it to the headers' text (names, return types, every argument, the structs above).
PROTOTYPES = {
    "camo_fusion.h": (
        ("camo_abi_version", i32, ()),
        ("camo_last_error", C.c_char_p, ()),
        ("camo_workspace_bytes", sz, (dims, i32, i32, i32)),
        ("camo_batch_desc_bytes", sz, (i32, i32)),
        ("camo_prepare_batch", i32, (vp, i32, i32, i32, vp, sz, vp)),
        ("camo_gather_batch", i32, (vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, u64, vp)),
        ("camo_forward", i32, (dims, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp, vp, i32, u64, i32, i32, vp)),
        ("camo_forward_cached", i32, (dims, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp, vp, i32, u64, i32, i32, vp, i32, P(i32), vp)),
        ("camo_backward", i32, (dims, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp, i32, i32, u64, i32, i32, vp)),
        ("camo_loss", i32, (vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp)),
        ("camo_grad_sumsq", i32, (vp, sz, vp, vp)),
        ("camo_clip_adamw", i32, (vp, vp, vp, vp, sz, vp, f32, f32, f32, f32, f32, f32, i32, i32, vp)),
        ("camo_shadow_bytes", sz, (dims,)),
        ("camo_clip_adamw_shadows", i32, (dims, vp, vp, vp, vp, vp, sz, vp, f32, f32, f32, f32, f32, f32, i32, i32, vp, vp)),
        ("camo_forward_loss_backward", i32, (dims, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, vp, vp, vp, vp, vp, i32, u64, i32, vp, vp, i32, vp)),
        ("camo_debug_gemm", i32, (vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp)),
        ("camo_debug_gemm_batch", i32, (vp, P(i32), P(f32), i32, i32, f32, u64, vp)),
        ("camo_debug_gemm16", i32, (vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, vp)),
        ("camo_debug_ws_offset", i64, (dims, i32, i32, i32, C.c_char_p)),
        ("camo_debug_plan", i32, (dims, i32, i32, i32, i32, i32, i32, i32, i32, i32, P(CamoPlan))),
        ("camo_options_init", i32, (P(CamoOptions),)),
        ("camo_options_set", i32, (P(CamoOptions), C.c_char_p, i32)),
        ("camo_debug_set_stamps", i32, (vp, i32)),
        ("camo_prof_begin", i32, (i32,)),
        ("camo_prof_end", i32, (P(f64), P(i32), P(f64))),
        ("camo_prof_kind", i32, (i32, P(f64), P(i32), P(f64))),
        ("camo_tail_timeouts", i32, (vp,)),
        ("camo_tail_poison_to_grads", i32, (vp, vp)),
    ),
    "camo_rg_gnn.h": (
        ("camo_rg_workspace_bytes", sz, (rgdims, i32)),
        ("camo_rg_build_csr", i32, (vp, vp, i32, i32, vp, vp, vp, vp, vp)),
        ("camo_rg_node_embeddings", i32, (rgdims, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp)),
    ),
    "camo_rg_features.h": (
        ("camo_rg_graph_workspace_bytes", sz, (i32,)),
        ("camo_rg_region_graph", i32, (vp, vp, vp, i32, i32, i32, vp, sz, vp, vp, vp, vp, i32, vp, vp)),
    ),
    "camo_rg_batch.h": (
        ("camo_rg_batch_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_rg_region_graph_batch", i32, (vp, vp, vp, i32, i32, i32, i32, vp, sz, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp)),
    ),
    "camo_canny.h": (
        ("camo_canny_workspace_bytes", sz, (i32, i32, i32)),
        ("camo_canny", i32, (vp, i32, i32, i32, f32, f32, f32, vp, sz, vp, vp, vp)),
        ("camo_canny_hysteresis", i32, (vp, i32, i32, i32, vp, sz, vp, vp)),
    ),
    "camo_slic.h": (
        ("camo_slic_grid", i32, (i32, i32, i32, P(i32))),
        ("camo_slic_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_slic", i32, (vp, i32, i32, i32, i32, f32, f32, vp, sz, vp, vp, vp)),
        ("camo_slic_preprocess", i32, (vp, i32, i32, i32, f32, f32, vp, vp)),
        ("camo_slic_assign", i32, (vp, vp, i32, i32, i32, i32, i32, vp, vp, vp)),
        ("camo_slic_update", i32, (vp, vp, i32, i32, i32, i32, vp, vp, vp)),
        ("camo_slic_connect", i32, (vp, i32, i32, i32, i32, i32, vp, sz, vp, vp, vp)),
    ),
    "camo_rg_detect.h": (
        ("camo_rg_node_heads", i32, (rgdims, i32, vp, vp, i32, vp, vp, vp)),
        ("camo_rg_paint", i32, (vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp)),
        ("camo_seg_counts", i32, (vp, i64, vp, f32, i32, i32, i32, vp, vp)),
    ),
    "camo_rg_train.h": (
        ("camo_rg_train_workspace_bytes", sz, (rgdims, i32, i32, i32)),
        ("camo_rg_loss_backward", i32, (rgdims, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, f32, f32, f32, vp, sz, vp, vp, vp)),
    ),
    "camo_rg_train_bn.h": (
        ("camo_rg_train_bn_workspace_bytes", sz, (rgdims, i32, i32, i32)),
        ("camo_rg_loss_backward_bn", i32, (rgdims, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, f32, f32, f32, vp, sz, vp, vp, f32, vp, vp, vp)),
    ),
    "camo_rg_train_drop.h": (
        ("camo_rg_train_drop_workspace_bytes", sz, (rgdims, i32, i32, i32, i32)),
        ("camo_rg_loss_backward_drop", i32, (rgdims, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, f32, f32, f32, vp, sz, vp, vp, f32, vp, vp,
                                             i32, f32, f32, f32, u64, vp)),
    ),
    "camo_rg_targets.h": (
        ("camo_rg_node_targets", i32, (vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp)),
    ),
    "camo_rg_pixel_loss.h": (
        ("camo_rg_pixel_weights", i32, (vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp)),
        ("camo_rg_loss_backward_pixel", i32, (rgdims, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, f32, f32, f32, vp, sz, vp, vp, f32, vp, vp,
                                              i32, f32, f32, f32, u64, vp, vp, i32, i32, f32, vp)),
    ),
    "camo_seg_measures.h": (
        ("camo_seg_histograms", i32, (vp, i64, vp, i32, i32, i32, vp, vp, vp)),
        ("camo_seg_weighted_f_workspace_bytes", sz, (i32, i32, i32)),
        ("camo_seg_weighted_f", i32, (vp, i64, vp, i32, i32, i32, vp, vp, sz, vp, vp)),
    ),
    "camo_resize.h": (
        ("camo_resize", i32, (vp, i64, i32, vp, i64, i32, vp, i32, i32, i32, i64, vp, vp)),
    ),
    "camo_instances.h": (
        ("camo_instances_workspace_bytes", sz, (i32, i32, i32)),
        ("camo_instances", i32, (vp, i64, f32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp)),
    ),
    "camo_inst_match.h": (
        ("camo_inst_match_workspace_bytes", sz, (i32, i32, i32, i32, i32, i32)),
        ("camo_inst_match", i32, (vp, vp, i32, i32, i32, i32, i32, vp, i32, P(i32), i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp)),
    ),
    "camo_boundary.h": (
        ("camo_boundary_labels_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_boundary_labels", i32, (vp, i32, i32, i32, i32, vp, vp, sz, vp)),
        ("camo_boundary_match_workspace_bytes", sz, (i32, i32, i32, i32, i32, i32)),
        ("camo_boundary_match", i32, (vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, P(i32), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp)),
    ),
    "camo_guided.h": (
        ("camo_guided_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_guided_filter", i32, (vp, vp, i64, i32, i32, i32, i32, i32, f64, i32, vp, vp, vp, sz, vp)),
        ("camo_guided_apply", i32, (vp, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, i32, vp, vp)),
    ),
    "camo_rle.h": (
        ("camo_rle_runs_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_rle_runs", i32, (vp, i32, i32, i32, i32, vp, vp, vp, sz, vp)),
        ("camo_rle_decode_workspace_bytes", sz, (i32, i32, i32, i32, i32)),
        ("camo_rle_decode", i32, (vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp)),
    ),
    "camo_poly.h": (
        ("camo_poly_decode_workspace_bytes", sz, (i32, i32, i32, i32, i32, i32)),
        ("camo_poly_decode", i32, (vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp)),
    ),
    "camo_contours.h": (
        ("camo_contours_workspace_bytes", sz, (i32, i32, i32, i32, i32, i32)),
        ("camo_contours", i32, (vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp)),
    ),
    "camo_split.h": (
        ("camo_split_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_split_instances", i32, (vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp)),
    ),
    "camo_split_geo.h": (
        ("camo_split_geodesic_workspace_bytes", sz, (i32, i32, i32, i32)),
        ("camo_split_instances_geodesic", i32, (vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp, i32, vp)),
        ("camo_split_geodesic_resume", i32, (vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp, i32, vp)),
    ),
    "camo_split_merge.h": (
        ("camo_split_merge_workspace_bytes", sz, (i32, i32, i32)),
        ("camo_split_merge", i32, (vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp)),
    ),
    "camo_augment.h": (
        ("camo_augment_workspace_bytes", sz, (i32, i32, i32, i32, i32)),
        ("camo_augment", i32, (vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp)),
    ),
}


def symbols(header):
    """The names ``include/<header>`` declares, in its order."""
    return tuple(name for name, _, _ in PROTOTYPES[header])


SYMBOLS = symbols("camo_fusion.h")


class CamoError(RuntimeError):
    pass


_lib = None


def _set_option_everywhere(name, value):
    from . import engine
    return engine.set_option_all(name.decode() if isinstance(name, bytes) else name, int(value))


def lib():
    """The loaded library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CamoError(f"{LIB_PATH} is missing: the HIP extension has not been built and there is no CPU "
                        "fallback. Run `python -m camouflage_multimodal_amd.build` (needs hipcc).")
    L = C.CDLL(LIB_PATH)
    for header, protos in PROTOTYPES.items():
        for name, restype, argtypes in protos:
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise CamoError(f"{LIB_PATH} does not export {name} (include/{header}): it is older than this package; "
                                "rebuild it with `python -m camouflage_multimodal_amd.build`") from None
            fn.restype, fn.argtypes = restype, list(argtypes)
    # tests and developer tools switch schedules "for the process": a Python-side convenience that sets the option on every live
    # engine and on the defaults of engines created later (engine.set_option_all) -- the library itself keeps no option state
    L.camo_debug_set_option = _set_option_everywhere
    v = L.camo_abi_version()
    if v != ABI_VERSION:
        raise CamoError(f"libcamo_fusion.so has ABI version {v}, this package expects {ABI_VERSION}: rebuild it")
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().camo_last_error().decode("utf-8", "replace")
        raise CamoError(f"{what or 'camo call'} failed (code {rc}): {msg}")


def require_device(t, name):
    """The product path runs on a HIP device only."""
    if not t.is_cuda:
        raise CamoError(f"{name} is on {t.device}: the fusion path runs as HIP kernels on an MI355X and has no CPU "
                        "fallback (move the model and its inputs to 'cuda').")


# ---- what every wrapper of a library call repeats, stated once.  torch is imported where a function needs it, so
# this module still imports without it.  The fusion engine's step path (engine.py, optim.py, losses.py) takes the two pointers from
# here and nothing else: it caches its sizes, and a Python call level is time it has not got.

def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_torch = _raw_stream = None


def _bind_torch():
    """torch and its raw-stream getter, bound at ``_stream_ptr``'s first call: the engine's step pays no import statement per call."""
    global _torch, _raw_stream
    import torch
    _torch, _raw_stream = torch, getattr(torch._C, "_cuda_getCurrentRawStream", None)
    return torch


def _stream_ptr(device=None):
    """The current HIP stream of ``device`` (default: the current device) as a void*."""
    torch = _torch or _bind_torch()
    if _raw_stream is not None:                              # (a plain C call: ~0.3 us against ~8 us for torch.cuda.current_stream())
        idx = device.index if isinstance(device, torch.device) and device.index is not None else torch.cuda.current_device()
        return C.c_void_p(_raw_stream(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(entry, device, *args):
    """The library's ``entry(*args)`` with ``device`` current, then ``check``: the name is stated once.  The stream is one of
    ``args``, where the entry's prototype has it."""
    import torch
    with torch.cuda.device(device):
        rc = getattr(lib(), entry)(*args)
    check(rc, entry)


def workspace(bytes_entry, *args, device, refuse=None):
    """(a uint8 buffer on ``device`` of the size the library's ``bytes_entry(*args)`` states, that size).  0 is the library's answer
    to arguments it does not take: ``refuse()``, the call site's exception, is raised then -- ``None`` raises ``CamoError`` with the
    library's own words (``check``), ``False`` says that 0 is a valid answer here, and the buffer is then one byte."""
    import torch
    need = int(getattr(lib(), bytes_entry)(*args))
    if need == 0 and refuse is not False:
        if refuse is None:
            check(-1, bytes_entry)
        raise refuse()
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device), need


def image_planes(t):
    """A prediction map [N, H, W] as (fp32 tensor the library reads in place through its image stride, that stride): one channel of a
    [N, C, H, W] map stays where it is, anything else is made contiguous; the stride of a single image is H W."""
    import torch
    N, H, W = t.shape
    t = t.detach()
    if t.dtype != torch.float32 or t.stride(2) != 1 or t.stride(1) != W or (N > 1 and t.stride(0) < H * W):
        t = t.to(torch.float32).contiguous()
    return t, (t.stride(0) if N > 1 else H * W)


def label_map(t, name):
    """An int32 label map [N, H, W], or [H, W] as N = 1; the ``ValueError`` of anything else names the argument."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"need {name} [N, H, W] or [H, W] with at least one pixel, got {tuple(t.shape)}")
    if t.dtype != torch.int32:
        raise ValueError(f"{name} must be int32, got {t.dtype}")
    return t


def tail_timeouts(device=None):
    """Number of arrival waits of the one-launch tail kernel that gave up on ``device`` (default: the current HIP device) since the
    library was loaded (synchronous; see camo_tail_timeouts in include/camo_fusion.h).  A step that hit one is not applied: its
    loss terms are NaN and the optimizer kernels skip an update whose gradient norm is not finite."""
    n = C.c_uint32(0)
    if device is not None:
        import torch
        with torch.cuda.device(device):
            check(lib().camo_tail_timeouts(C.byref(n)), "camo_tail_timeouts")
    else:
        check(lib().camo_tail_timeouts(C.byref(n)), "camo_tail_timeouts")
    return int(n.value)
