// C ABI of the image pipeline around the detector (include/camo_instances.h, camo_inst_match.h, camo_boundary.h, camo_guided.h,
// camo_rle.h, camo_poly.h, camo_contours.h, camo_split.h, camo_split_geo.h, camo_split_merge.h): argument checks, workspace carving and the launchers' calls.  No device code here.
#include <hip/hip_runtime.h>

#include <cmath>

#include "abi_util.h"
#include "instances.h"
#include "inst_match.h"
#include "boundary.h"
#include "guided.h"
#include "rle.h"
#include "poly.h"
#include "contours.h"
#include "split.h"
#include "../../include/camo_rg_detect.h"
#include "../../include/camo_instances.h"
#include "../../include/camo_inst_match.h"
#include "../../include/camo_boundary.h"
#include "../../include/camo_guided.h"
#include "../../include/camo_rle.h"
#include "../../include/camo_poly.h"
#include "../../include/camo_contours.h"
#include "../../include/camo_split.h"
#include "../../include/camo_split_geo.h"
#include "../../include/camo_split_merge.h"

using namespace camo_abi;

extern "C" {

// ---- Object instances of a predicted mask (include/camo_instances.h) ---------------------------------------------
static int inst_check(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if (N > CAMO_RGD_MAX_IMAGES) return fail(CAMO_E_ARG, "N exceeds CAMO_RGD_MAX_IMAGES");
  if ((long long)H * W > CAMO_RGD_MAX_IMAGE_PIXELS) return fail(CAMO_E_ARG, "H * W exceeds CAMO_RGD_MAX_IMAGE_PIXELS");
  if ((long long)N * H * W > CAMO_RGD_MAX_PIXELS) return fail(CAMO_E_ARG, "N * H * W exceeds CAMO_RGD_MAX_PIXELS (32-bit pixel indices)");
  return 0;
}

size_t camo_instances_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (inst_check(N, H, W)) return 0;
  return inst_carve(N, H, W, nullptr).bytes;
}

int camo_instances(const float* pred, int64_t pred_image_stride, float threshold, int32_t N, int32_t H, int32_t W, int32_t connectivity,
                   int32_t min_area, int32_t fill_holes, int32_t max_instances, int32_t* labels, uint8_t* clean, int64_t* table,
                   int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (int e = inst_check(N, H, W)) return e;
  if (connectivity != 4 && connectivity != 8) return fail(CAMO_E_ARG, "connectivity must be 4 or 8");
  if (min_area < 0) return fail(CAMO_E_ARG, "min_area must be >= 0");
  if (max_instances < 1) return fail(CAMO_E_ARG, "max_instances must be >= 1");
  if ((long long)N * max_instances > CAMO_INST_MAX_ROWS) return fail(CAMO_E_ARG, "N * max_instances exceeds CAMO_INST_MAX_ROWS");
  if (pred_image_stride < (long long)H * W) return fail(CAMO_E_ARG, "pred_image_stride must be >= H * W");
  if (!std::isfinite(threshold)) return fail(CAMO_E_ARG, "threshold must be finite");
  if (!pred || !labels || !clean || !table || !counts || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(CAMO_E_ARG, "table must be 8-byte aligned");
  const InstWs w = inst_carve(N, H, W, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_instances_workspace_bytes")) return e;
  CK(launch_instances(pred, pred_image_stride, threshold, N, H, W, connectivity, min_area, fill_holes != 0, max_instances, w, labels, clean,
                      reinterpret_cast<long long*>(table), counts, static_cast<hipStream_t>(stream)), "instances");
  return 0;
}

// ---- Instance matching: overlap table and greedy matches (include/camo_inst_match.h) -----------------------------
static int im_check(int N, int H, int W, int P, int G, int T) {
  if (int e = inst_check(N, H, W)) return e;
  if (P < 1 || P > CAMO_IM_MAX_IDS) return fail(CAMO_E_ARG, "P must be in [1, CAMO_IM_MAX_IDS]");
  if (G < 1 || G > CAMO_IM_MAX_IDS) return fail(CAMO_E_ARG, "G must be in [1, CAMO_IM_MAX_IDS]");
  if ((long long)N * (P + 1) * (G + 1) > CAMO_IM_MAX_CELLS) return fail(CAMO_E_ARG, "N * (P + 1) * (G + 1) exceeds CAMO_IM_MAX_CELLS");
  if (T < 1 || T > CAMO_IM_MAX_THRESHOLDS) return fail(CAMO_E_ARG, "T must be in [1, CAMO_IM_MAX_THRESHOLDS]");
  return 0;
}

// What camo_inst_match and camo_boundary_match check first, in this order: the sizes, the thresholds (into thr), the table.
static int im_args(int N, int H, int W, int P, int G, int T, const int32_t* thr_num, int thr_den, const int64_t* pred_table, int pred_table_rows,
                   ImThresholds* thr) {
  if (int e = im_check(N, H, W, P, G, T)) return e;
  if (!thr_num) return fail(CAMO_E_ARG, "thr_num is null");
  if (thr_den < 1 || thr_den > 1000) return fail(CAMO_E_ARG, "thr_den must be in [1, 1000]");
  thr->den = thr_den;
  for (int k = 0; k < T; ++k) {
    if (thr_num[k] < 1 || thr_num[k] > thr_den) return fail(CAMO_E_ARG, "every thr_num must be in [1, thr_den]");
    thr->num[k] = thr_num[k];
  }
  if (pred_table && pred_table_rows < 1) return fail(CAMO_E_ARG, "pred_table_rows must be >= 1 when pred_table is given");
  if (reinterpret_cast<uintptr_t>(pred_table) & 7) return fail(CAMO_E_ARG, "pred_table must be 8-byte aligned");
  return 0;
}

size_t camo_inst_match_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t P, int32_t G, int32_t T) {
  if (im_check(N, H, W, P, G, T)) return 0;
  return im_carve(N, P, G, false, nullptr).bytes;
}

int camo_inst_match(const int32_t* pred_labels, const int32_t* gt_labels, int32_t N, int32_t H, int32_t W, int32_t P, int32_t G,
                    const int64_t* pred_table, int32_t pred_table_rows, const int32_t* thr_num, int32_t thr_den, int32_t T, int32_t* inter,
                    int32_t* pred_rows, int32_t* gt_area, int32_t* match, int32_t* gt_match, int32_t* counts, void* ws, size_t ws_bytes,
                    void* stream) {
  ImThresholds thr{};
  if (int e = im_args(N, H, W, P, G, T, thr_num, thr_den, pred_table, pred_table_rows, &thr)) return e;
  if (!pred_labels || !gt_labels || !inter || !pred_rows || !gt_area || !match || !gt_match || !counts || !ws)
    return fail(CAMO_E_ARG, "null pointer argument");
  const ImWs w = im_carve(N, P, G, false, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_inst_match_workspace_bytes")) return e;
  CK(launch_inst_match(pred_labels, gt_labels, N, H, W, P, G, reinterpret_cast<const long long*>(pred_table), pred_table ? pred_table_rows : 0,
                       thr, T, w, inter, pred_rows, gt_area, match, gt_match, counts, static_cast<hipStream_t>(stream)), "inst match");
  return 0;
}

// ---- Boundary IoU: boundary regions of a label map, match under min(mask IoU, boundary IoU) (include/camo_boundary.h) ---
static_assert(BD_STRIP == CAMO_BD_STRIP, "include/camo_boundary.h states the kernel's constant");

static int bd_check(int N, int H, int W, int d) {
  if (int e = inst_check(N, H, W)) return e;
  if (d < 1 || d > CAMO_BD_MAX_DISTANCE) return fail(CAMO_E_ARG, "d must be in [1, CAMO_BD_MAX_DISTANCE]");
  return 0;
}

size_t camo_boundary_labels_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t d) {
  if (bd_check(N, H, W, d)) return 0;
  return ((size_t)N * H * W + 255) & ~size_t(255);
}

int camo_boundary_labels(const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t d, int32_t* out, void* ws, size_t ws_bytes,
                         void* stream) {
  if (int e = bd_check(N, H, W, d)) return e;
  if (!labels) return fail(CAMO_E_ARG, "labels is null");
  if (!out) return fail(CAMO_E_ARG, "out is null");
  if (!ws) return fail(CAMO_E_ARG, "ws is null");
  const uintptr_t a = reinterpret_cast<uintptr_t>(labels), b = reinterpret_cast<uintptr_t>(out), bytes = (uintptr_t)N * H * W * 4;
  if (a < b + bytes && b < a + bytes) return fail(CAMO_E_ARG, "labels and out must not overlap");
  if (int e = ws_check(ws, ws_bytes, camo_boundary_labels_workspace_bytes(N, H, W, d), "camo_boundary_labels_workspace_bytes")) return e;
  CK(launch_boundary_labels(labels, N, H, W, d, out, static_cast<unsigned char*>(ws), static_cast<hipStream_t>(stream)), "boundary labels");
  return 0;
}

size_t camo_boundary_match_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t P, int32_t G, int32_t T) {
  if (im_check(N, H, W, P, G, T)) return 0;
  return im_carve(N, P, G, true, nullptr).bytes;
}

int camo_boundary_match(const int32_t* pred_labels, const int32_t* gt_labels, const int32_t* pred_bd, const int32_t* gt_bd, int32_t N, int32_t H,
                        int32_t W, int32_t P, int32_t G, const int64_t* pred_table, int32_t pred_table_rows, const int32_t* thr_num, int32_t thr_den,
                        int32_t T, int32_t* inter, int32_t* inter_bd, int32_t* pred_rows, int32_t* gt_area, int32_t* match, int32_t* gt_match,
                        int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  ImThresholds thr{};
  if (int e = im_args(N, H, W, P, G, T, thr_num, thr_den, pred_table, pred_table_rows, &thr)) return e;
  if (!pred_labels || !gt_labels || !pred_bd || !gt_bd || !inter || !inter_bd || !pred_rows || !gt_area || !match || !gt_match || !counts || !ws)
    return fail(CAMO_E_ARG, "null pointer argument");
  const ImWs w = im_carve(N, P, G, true, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_boundary_match_workspace_bytes")) return e;
  CK(launch_boundary_match(pred_labels, gt_labels, pred_bd, gt_bd, N, H, W, P, G, reinterpret_cast<const long long*>(pred_table),
                           pred_table ? pred_table_rows : 0, thr, T, w, inter, inter_bd, pred_rows, gt_area, match, gt_match, counts,
                           static_cast<hipStream_t>(stream)), "boundary match");
  return 0;
}

// ---- Instance splitter: distance-transform cores, nearest-core cells (include/camo_split.h) -------------------------
static int split_check(int N, int H, int W, int max_split) {
  if (int e = inst_check(N, H, W)) return e;
  if (H > CAMO_SEG_WF_MAX_SIDE || W > CAMO_SEG_WF_MAX_SIDE) return fail(CAMO_E_ARG, "H and W must be at most CAMO_SEG_WF_MAX_SIDE");
  if (max_split < 1 || max_split > CAMO_SPLIT_MAX_SPLIT) return fail(CAMO_E_ARG, "max_split must be in [1, CAMO_SPLIT_MAX_SPLIT]");
  return 0;
}

size_t camo_split_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t max_split) {
  if (split_check(N, H, W, max_split)) return 0;
  return split_carve(N, H, W, max_split, nullptr).bytes;
}

// What the three calls check before the workspace, in this order.
static int split_args(const int32_t* labels, const float* pred, int64_t pred_image_stride, int N, int H, int W, int ratio_num, int ratio_den,
                      int min_core, int max_split, int max_instances, const int32_t* out_labels, const int64_t* table, const int32_t* counts,
                      const void* ws) {
  if (int e = split_check(N, H, W, max_split)) return e;
  if (ratio_den < 2 || ratio_den > CAMO_SPLIT_MAX_DEN) return fail(CAMO_E_ARG, "ratio_den must be in [2, CAMO_SPLIT_MAX_DEN]");
  if (ratio_num < 1 || ratio_num >= ratio_den) return fail(CAMO_E_ARG, "ratio_num must be in [1, ratio_den)");
  if (min_core < 0) return fail(CAMO_E_ARG, "min_core must be >= 0");
  if (max_instances < 1) return fail(CAMO_E_ARG, "max_instances must be >= 1");
  if ((long long)N * max_instances > CAMO_INST_MAX_ROWS) return fail(CAMO_E_ARG, "N * max_instances exceeds CAMO_INST_MAX_ROWS");
  if (pred && pred_image_stride < (long long)H * W) return fail(CAMO_E_ARG, "pred_image_stride must be >= H * W");
  if (!labels) return fail(CAMO_E_ARG, "labels is null");
  if (!out_labels || !table || !counts || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(CAMO_E_ARG, "table must be 8-byte aligned");
  const uintptr_t a = reinterpret_cast<uintptr_t>(labels), b = reinterpret_cast<uintptr_t>(out_labels), bytes = (uintptr_t)N * H * W * 4;
  if (a < b + bytes && b < a + bytes) return fail(CAMO_E_ARG, "labels and out_labels must not overlap");
  return 0;
}

int camo_split_instances(const int32_t* labels, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W, int32_t ratio_num,
                         int32_t ratio_den, int32_t min_core, int32_t max_split, int32_t max_instances, int32_t* out_labels, int64_t* table,
                         int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (int e = split_args(labels, pred, pred_image_stride, N, H, W, ratio_num, ratio_den, min_core, max_split, max_instances, out_labels, table, counts, ws))
    return e;
  const SplitWs w = split_carve(N, H, W, max_split, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_split_workspace_bytes")) return e;
  CK(launch_split(labels, pred, pred_image_stride, N, H, W, ratio_num, ratio_den, min_core, max_split, max_instances, w, out_labels,
                  reinterpret_cast<long long*>(table), counts, static_cast<hipStream_t>(stream)), "split instances");
  return 0;
}

// ---- Geodesic growth for the splitter: connected parts from cores (include/camo_split_geo.h) -----------------------
size_t camo_split_geodesic_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t max_split) {
  if (split_check(N, H, W, max_split)) return 0;
  return split_geo_carve(N, H, W, max_split, nullptr).bytes;
}

static int split_geo_args(const int32_t* labels, const float* pred, int64_t pred_image_stride, int N, int H, int W, int ratio_num, int ratio_den,
                          int min_core, int max_split, int max_instances, const int32_t* out_labels, const int64_t* table, const int32_t* counts,
                          void* ws, size_t ws_bytes, int rounds, const int32_t* pending, SplitGeoWs* w) {
  if (int e = split_args(labels, pred, pred_image_stride, N, H, W, ratio_num, ratio_den, min_core, max_split, max_instances, out_labels, table, counts, ws))
    return e;
  if (rounds < 1 || rounds > CAMO_SPLIT_GEO_MAX_ROUNDS) return fail(CAMO_E_ARG, "rounds must be in [1, CAMO_SPLIT_GEO_MAX_ROUNDS]");
  if (!pending) return fail(CAMO_E_ARG, "pending is null");
  *w = split_geo_carve(N, H, W, max_split, ws);
  return ws_check(ws, ws_bytes, w->bytes, "camo_split_geodesic_workspace_bytes");
}

int camo_split_instances_geodesic(const int32_t* labels, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W,
                                  int32_t ratio_num, int32_t ratio_den, int32_t min_core, int32_t max_split, int32_t max_instances,
                                  int32_t* out_labels, int64_t* table, int32_t* counts, void* ws, size_t ws_bytes, void* stream, int32_t rounds,
                                  int32_t* pending) {
  SplitGeoWs w;
  if (int e = split_geo_args(labels, pred, pred_image_stride, N, H, W, ratio_num, ratio_den, min_core, max_split, max_instances, out_labels, table, counts,
                             ws, ws_bytes, rounds, pending, &w))
    return e;
  CK(launch_split_geo(labels, pred, pred_image_stride, N, H, W, ratio_num, ratio_den, min_core, max_split, max_instances, rounds, w, out_labels,
                      reinterpret_cast<long long*>(table), counts, pending, static_cast<hipStream_t>(stream)), "split instances, geodesic");
  return 0;
}

int camo_split_geodesic_resume(const int32_t* labels, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W, int32_t ratio_num,
                               int32_t ratio_den, int32_t min_core, int32_t max_split, int32_t max_instances, int32_t* out_labels, int64_t* table,
                               int32_t* counts, void* ws, size_t ws_bytes, void* stream, int32_t rounds, int32_t* pending) {
  SplitGeoWs w;
  if (int e = split_geo_args(labels, pred, pred_image_stride, N, H, W, ratio_num, ratio_den, min_core, max_split, max_instances, out_labels, table, counts,
                             ws, ws_bytes, rounds, pending, &w))
    return e;
  CK(launch_split_geo_resume(labels, pred, pred_image_stride, N, H, W, max_instances, rounds, w, out_labels, reinterpret_cast<long long*>(table), counts,
                             pending, static_cast<hipStream_t>(stream)), "split instances, geodesic resume");
  return 0;
}

// ---- Low-dynamic cores merged: a post-pass on either growth's part map (include/camo_split_merge.h) ----------------
size_t camo_split_merge_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (split_check(N, H, W, 1)) return 0;
  return split_merge_carve(N, H, W, nullptr).bytes;
}

int camo_split_merge(const int32_t* labels, const int32_t* parts, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W,
                     int32_t merge_num, int32_t merge_den, int32_t max_instances, int32_t* out_labels, int64_t* table, int32_t* counts, void* ws,
                     size_t ws_bytes, void* stream) {
  if (int e = split_check(N, H, W, 1)) return e;
  if (merge_den < 1 || merge_den > CAMO_SPLIT_MAX_DEN) return fail(CAMO_E_ARG, "merge_den must be in [1, CAMO_SPLIT_MAX_DEN]");
  if (merge_num < 1 || merge_num > merge_den) return fail(CAMO_E_ARG, "merge_num must be in [1, merge_den]");
  if (max_instances < 1) return fail(CAMO_E_ARG, "max_instances must be >= 1");
  if ((long long)N * max_instances > CAMO_INST_MAX_ROWS) return fail(CAMO_E_ARG, "N * max_instances exceeds CAMO_INST_MAX_ROWS");
  if (pred && pred_image_stride < (long long)H * W) return fail(CAMO_E_ARG, "pred_image_stride must be >= H * W");
  if (!labels) return fail(CAMO_E_ARG, "labels is null");
  if (!parts) return fail(CAMO_E_ARG, "parts is null");
  if (!out_labels || !table || !counts || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(CAMO_E_ARG, "table must be 8-byte aligned");
  const uintptr_t a = reinterpret_cast<uintptr_t>(labels), p = reinterpret_cast<uintptr_t>(parts), b = reinterpret_cast<uintptr_t>(out_labels),
                  bytes = (uintptr_t)N * H * W * 4;
  if (a < b + bytes && b < a + bytes) return fail(CAMO_E_ARG, "labels and out_labels must not overlap");
  if (p < b + bytes && b < p + bytes) return fail(CAMO_E_ARG, "parts and out_labels must not overlap");
  const SplitMergeWs w = split_merge_carve(N, H, W, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_split_merge_workspace_bytes")) return e;
  CK(launch_split_merge(labels, parts, pred, pred_image_stride, N, H, W, merge_num, merge_den, max_instances, w, out_labels,
                        reinterpret_cast<long long*>(table), counts, static_cast<hipStream_t>(stream)), "split merge");
  return 0;
}

// ---- Edge-aware mask refinement: guided filter and native-size apply (include/camo_guided.h) ---------------------
static int gf_check(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if (N > CAMO_RGD_MAX_IMAGES) return fail(CAMO_E_ARG, "N exceeds CAMO_RGD_MAX_IMAGES");
  if (H > CAMO_RSZ_MAX_SIDE || W > CAMO_RSZ_MAX_SIDE) return fail(CAMO_E_ARG, "H or W exceeds CAMO_RSZ_MAX_SIDE");
  if ((long long)H * W > CAMO_RGD_MAX_IMAGE_PIXELS) return fail(CAMO_E_ARG, "H * W exceeds CAMO_RGD_MAX_IMAGE_PIXELS");
  if ((long long)N * H * W > CAMO_RGD_MAX_PIXELS) return fail(CAMO_E_ARG, "N * H * W exceeds CAMO_RGD_MAX_PIXELS");
  if (C != 1 && C != 3) return fail(CAMO_E_ARG, "C must be 1 (grey guide) or 3 (colour guide)");
  return 0;
}

size_t camo_guided_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (gf_check(N, H, W, C)) return 0;
  return gf_carve(N, H, W, C, nullptr).bytes;
}

int camo_guided_filter(const float* guide, const float* p, int64_t p_image_stride, int32_t N, int32_t H, int32_t W, int32_t C, int32_t radius,
                       double eps, int32_t clamp, float* q, float* coef, void* ws, size_t ws_bytes, void* stream) {
  if (int e = gf_check(N, H, W, C)) return e;
  if (radius < 1 || radius > CAMO_GF_MAX_RADIUS) return fail(CAMO_E_ARG, "radius must be in [1, CAMO_GF_MAX_RADIUS]");
  if (!(eps >= CAMO_GF_MIN_EPS && eps <= CAMO_GF_MAX_EPS)) return fail(CAMO_E_ARG, "eps must be in [CAMO_GF_MIN_EPS, CAMO_GF_MAX_EPS]");
  if (clamp != 0 && clamp != 1) return fail(CAMO_E_ARG, "clamp must be 0 or 1");
  if (p_image_stride < (long long)H * W) return fail(CAMO_E_ARG, "p_image_stride must be >= H * W");
  if (!guide || !p || !q || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if ((reinterpret_cast<uintptr_t>(guide) | reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(coef)) & 3)
    return fail(CAMO_E_ARG, "guide, p, q and coef must be 4-byte aligned");
  const GfWs w = gf_carve(N, H, W, C, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_guided_workspace_bytes")) return e;
  CK(launch_guided_filter(guide, p, p_image_stride, N, H, W, C, radius, eps, clamp != 0, q, coef, w, static_cast<hipStream_t>(stream)),
     "guided filter");
  return 0;
}

int camo_guided_apply(const float* coef, int32_t N, int32_t C, int32_t h, int32_t w, const uint8_t* guide, int64_t guide_elems, float* out,
                      int64_t out_elems, const int64_t* table, int64_t max_dst_pixels, int32_t clamp, int32_t* status, void* stream) {
  if (int e = gf_check(N, h, w, C)) return e;
  if (clamp != 0 && clamp != 1) return fail(CAMO_E_ARG, "clamp must be 0 or 1");
  if (guide_elems < 1) return fail(CAMO_E_ARG, "need guide_elems >= 1");
  if (out_elems < 1) return fail(CAMO_E_ARG, "need out_elems >= 1");
  if (max_dst_pixels < 1 || max_dst_pixels > CAMO_RGD_MAX_IMAGE_PIXELS) return fail(CAMO_E_ARG, "need 1 <= max_dst_pixels <= CAMO_RGD_MAX_IMAGE_PIXELS");
  if (!coef || !guide || !out || !table || !status) return fail(CAMO_E_ARG, "null pointer argument");
  if ((reinterpret_cast<uintptr_t>(coef) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(status)) & 3)
    return fail(CAMO_E_ARG, "coef, out and status must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(CAMO_E_ARG, "table must be 8-byte aligned");
  CK(launch_guided_apply(coef, N, C, h, w, guide, guide_elems, out, out_elems, reinterpret_cast<const long long*>(table), max_dst_pixels,
                         clamp != 0, status, static_cast<hipStream_t>(stream)), "guided apply");
  return 0;
}

// ---- COCO run-length masks: label maps to runs, counts to label maps (include/camo_rle.h) -------------------------
static int rle_runs_check(int N, int H, int W, int R) {
  if (int e = inst_check(N, H, W)) return e;
  if (R < 1) return fail(CAMO_E_ARG, "R must be >= 1");
  if ((long long)N * R > CAMO_RLE_MAX_ROWS) return fail(CAMO_E_ARG, "N * R exceeds CAMO_RLE_MAX_ROWS");
  return 0;
}

size_t camo_rle_runs_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t R) {
  if (rle_runs_check(N, H, W, R)) return 0;
  return rle_runs_carve(N, H, W, nullptr).bytes;
}

int camo_rle_runs(const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t R, int32_t* runs, int32_t* counts, void* ws, size_t ws_bytes,
                  void* stream) {
  if (int e = rle_runs_check(N, H, W, R)) return e;
  if (!labels || !runs || !counts || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(counts)) & 3) return fail(CAMO_E_ARG, "labels and counts must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(runs) & 7) return fail(CAMO_E_ARG, "runs must be 8-byte aligned");
  const RleRunsWs w = rle_runs_carve(N, H, W, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_rle_runs_workspace_bytes")) return e;
  CK(launch_rle_runs(labels, N, H, W, R, w, runs, counts, static_cast<hipStream_t>(stream)), "rle runs");
  return 0;
}

static int rle_decode_check(int N, int H, int W, int A, int total) {
  if (int e = inst_check(N, H, W)) return e;
  if (A < 1 || A > CAMO_RLE_MAX_ANNOTATIONS) return fail(CAMO_E_ARG, "A must be in [1, CAMO_RLE_MAX_ANNOTATIONS]");
  if (total < 0 || total > CAMO_RLE_MAX_COUNTS) return fail(CAMO_E_ARG, "total must be in [0, CAMO_RLE_MAX_COUNTS]");
  return 0;
}

size_t camo_rle_decode_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t A, int32_t total) {
  if (rle_decode_check(N, H, W, A, total)) return 0;
  return rle_decode_carve(total, nullptr).bytes;
}

int camo_rle_decode(const int32_t* cnts, int32_t total, const int32_t* ann_off, const int32_t* ann_image, const int32_t* ann_value, int32_t A,
                    int32_t N, int32_t H, int32_t W, int32_t* labels, int64_t* ann_sum, void* ws, size_t ws_bytes, void* stream) {
  if (int e = rle_decode_check(N, H, W, A, total)) return e;
  if ((!cnts && total > 0) || !ann_off || !ann_image || !ann_value || !labels || !ann_sum || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(ann_sum) & 7) return fail(CAMO_E_ARG, "ann_sum must be 8-byte aligned");
  const RleDecodeWs w = rle_decode_carve(total, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_rle_decode_workspace_bytes")) return e;
  CK(launch_rle_decode(cnts, total, ann_off, ann_image, ann_value, A, N, H, W, w, labels, reinterpret_cast<long long*>(ann_sum),
                       static_cast<hipStream_t>(stream)), "rle decode");
  return 0;
}

// ---- COCO polygon annotations to label maps (include/camo_poly.h) --------------------------------------------------
static int poly_check(int N, int H, int W, int A, int P, int V) {
  if (int e = inst_check(N, H, W)) return e;
  if (A < 1 || A > CAMO_POLY_MAX_ANNOTATIONS) return fail(CAMO_E_ARG, "A must be in [1, CAMO_POLY_MAX_ANNOTATIONS]");
  if (P < 0 || P > CAMO_POLY_MAX_POLYGONS) return fail(CAMO_E_ARG, "P must be in [0, CAMO_POLY_MAX_POLYGONS]");
  if (V < 0 || V > CAMO_POLY_MAX_VERTICES) return fail(CAMO_E_ARG, "V must be in [0, CAMO_POLY_MAX_VERTICES]");
  if ((long long)P * (((long long)H * W + 31) / 32) > CAMO_POLY_MAX_PLANE_WORDS) return fail(CAMO_E_ARG, "P * ceil(H W / 32) exceeds CAMO_POLY_MAX_PLANE_WORDS");
  return 0;
}

size_t camo_poly_decode_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t A, int32_t P, int32_t V) {
  if (poly_check(N, H, W, A, P, V)) return 0;
  return poly_carve(H, W, A, P, nullptr).bytes;
}

int camo_poly_decode(const double* xy, int32_t V, const int32_t* poly_off, int32_t P, const int32_t* ann_poly_off, const int32_t* ann_image,
                     const int32_t* ann_value, int32_t A, int32_t N, int32_t H, int32_t W, int32_t* labels, int64_t* ann_area, void* ws, size_t ws_bytes,
                     void* stream) {
  if (int e = poly_check(N, H, W, A, P, V)) return e;
  if ((!xy && V > 0) || !poly_off || !ann_poly_off || !ann_image || !ann_value || !labels || !ann_area || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if ((reinterpret_cast<uintptr_t>(xy) | reinterpret_cast<uintptr_t>(ann_area)) & 7) return fail(CAMO_E_ARG, "xy and ann_area must be 8-byte aligned");
  const PolyWs w = poly_carve(H, W, A, P, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_poly_decode_workspace_bytes")) return e;
  CK(launch_poly_decode(xy, V, poly_off, P, ann_poly_off, ann_image, ann_value, A, N, H, W, w, labels, reinterpret_cast<long long*>(ann_area),
                        static_cast<hipStream_t>(stream)), "poly decode");
  return 0;
}

// ---- Instance contours: label maps to rings of corner vertices (include/camo_contours.h) ---------------------------
static int contour_check(int N, int H, int W, int C, int R, int V) {
  if (int e = inst_check(N, H, W)) return e;
  if (C < 1 || C > 4ll * H * W) return fail(CAMO_E_ARG, "C must be in [1, 4 H W]");
  if (R < 1) return fail(CAMO_E_ARG, "R must be >= 1");
  if (V < 1) return fail(CAMO_E_ARG, "V must be >= 1");
  if ((long long)N * C > CAMO_CONTOUR_MAX_CRACKS) return fail(CAMO_E_ARG, "N * C exceeds CAMO_CONTOUR_MAX_CRACKS");
  if ((long long)N * R > CAMO_CONTOUR_MAX_RINGS) return fail(CAMO_E_ARG, "N * R exceeds CAMO_CONTOUR_MAX_RINGS");
  if ((long long)N * V > CAMO_CONTOUR_MAX_VERTICES) return fail(CAMO_E_ARG, "N * V exceeds CAMO_CONTOUR_MAX_VERTICES");
  return 0;
}

size_t camo_contours_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t R, int32_t V) {
  if (contour_check(N, H, W, C, R, V)) return 0;
  return contour_carve(N, H, W, C, nullptr).bytes;
}

int camo_contours(const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t connectivity, int32_t C, int32_t R, int32_t V, int64_t* rings,
                  int32_t* xy, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (int e = contour_check(N, H, W, C, R, V)) return e;
  if (connectivity != 4 && connectivity != 8) return fail(CAMO_E_ARG, "connectivity must be 4 or 8");
  if (!labels || !rings || !xy || !counts || !ws) return fail(CAMO_E_ARG, "null pointer argument");
  if ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(counts)) & 3) return fail(CAMO_E_ARG, "labels and counts must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(rings) | reinterpret_cast<uintptr_t>(xy)) & 7) return fail(CAMO_E_ARG, "rings and xy must be 8-byte aligned");
  const ContourWs w = contour_carve(N, H, W, C, ws);
  if (int e = ws_check(ws, ws_bytes, w.bytes, "camo_contours_workspace_bytes")) return e;
  CK(launch_contours(labels, N, H, W, connectivity, C, R, V, w, reinterpret_cast<long long*>(rings), xy, counts, static_cast<hipStream_t>(stream)),
     "contours");
  return 0;
}
}  // extern "C"
