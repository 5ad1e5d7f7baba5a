// Instance matching (inst_match.hip, include/camo_inst_match.h) under mask IoU, and under min(mask IoU, boundary IoU)
// (include/camo_boundary.h): what the kernels, the launchers and the entry points share.  The launchers return
// hipError_t as int.
#pragma once
#include "common.h"

constexpr int IM_MAX_THRESHOLDS = 16;      // CAMO_IM_MAX_THRESHOLDS

struct ImWs {
  int* area_p;             // [N][P + 1] row sums of inter
  int* area_g;             // [N][G + 1] column sums of inter
  int* rank;               // [N][P] 0-based rank of predicted id p (at p - 1) in score order
  // the combined match only
  int* bd_area_p;          // [N][P + 1] row sums of inter_bd
  int* bd_area_g;          // [N][G + 1] column sums of inter_bd
  int* bd_counts;          // [N][CAMO_IM_COUNTS] the boundary maps' out-of-range pixels: counted, not reported
  size_t bytes;
};
ImWs im_carve(int N, int P, int G, bool boundary, void* base);

// the thresholds travel as a kernel argument: no device copy of the caller's host array
struct ImThresholds { int num[IM_MAX_THRESHOLDS]; int den; };

// Clear, overlap and areas of ONE table (three launches): inter [N][P + 1][G + 1] of the two maps, its row sums to area_p and to the
// first of every row_fields ints of pred_rows, its column sums to area_g and to every gt_fields-th int of gt_area, the pixels with a
// label out of range to counts [N][CAMO_IM_COUNTS] (which the clear zeroes).  with_rank: the score order too, to rank and to the second
// int of every row of pred_rows.  camo_inst_match's first three launches; camo_boundary_match runs it once per table.
int launch_im_table(const int* pred_labels, const int* gt_labels, int N, int H, int W, int P, int G, const long long* pred_table,
                    int pred_table_rows, bool with_rank, int* area_p, int* area_g, int* rank, int* inter, int* pred_rows, int row_fields,
                    int* gt_area, int gt_fields, int* counts, hipStream_t stream);

int launch_inst_match(const int* pred_labels, const int* gt_labels, int N, int H, int W, int P, int G, const long long* pred_table,
                      int pred_table_rows, const ImThresholds& thr, int T, const ImWs& ws, int* inter, int* pred_rows, int* gt_area,
                      int* match, int* gt_match, int* counts, hipStream_t stream);

// ws: im_carve with boundary
int launch_boundary_match(const int* pred_labels, const int* gt_labels, const int* pred_bd, const int* gt_bd, int N, int H, int W, int P, int G,
                          const long long* pred_table, int pred_table_rows, const ImThresholds& thr, int T, const ImWs& ws, int* inter,
                          int* inter_bd, int* pred_rows, int* gt_area, int* match, int* gt_match, int* counts, hipStream_t stream);

#ifdef __HIPCC__
// A candidate ground-truth id with its intersection i and union u; g == 0: none.  a before b: higher IoU, then smaller id.
struct ImCand { int i, u, g; };
__device__ __forceinline__ bool im_before(const ImCand& a, const ImCand& b) {
  if (a.g == 0) return false;
  if (b.g == 0) return true;
  const long long l = (long long)a.i * b.u, r = (long long)b.i * a.u;
  return l > r || (l == r && a.g < b.g);
}
// The smaller of the mask IoU i / u and the boundary IoU ib / ub of ground-truth id g, as a candidate: 0 / 1 when ub is 0, the mask
// fraction when they are equal.  Every factor is at most 2^27.
__device__ __forceinline__ ImCand bd_cand(int i, int u, int ib, int ub, int g) {
  if (ub == 0) return ImCand{0, 1, g};
  return (long long)i * ub <= (long long)ib * u ? ImCand{i, u, g} : ImCand{ib, ub, g};
}
// the wave's best candidate, in every lane
__device__ __forceinline__ ImCand im_wave_best(ImCand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const ImCand other{__shfl_xor(c.i, o, 64), __shfl_xor(c.u, o, 64), __shfl_xor(c.g, o, 64)};
    if (im_before(other, c)) c = other;
  }
  return c;
}
#endif
