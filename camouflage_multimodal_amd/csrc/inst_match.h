// Instance matching (inst_match.hip, include/camo_inst_match.h): what the kernels, the launcher and the entry points
// share.  The launcher returns hipError_t as int.
#pragma once
#include "common.h"

constexpr int IM_MAX_THRESHOLDS = 16;      // CAMO_IM_MAX_THRESHOLDS

struct ImWs {
  int* area_p;             // [N][P + 1] row sums of inter
  int* area_g;             // [N][G + 1] column sums of inter
  int* rank;               // [N][P] 0-based rank of predicted id p (at p - 1) in score order
  size_t bytes;
};
ImWs im_carve(int N, int P, int G, void* base);

// the thresholds travel as a kernel argument: no device copy of the caller's host array
struct ImThresholds { int num[IM_MAX_THRESHOLDS]; int den; };

int launch_inst_match(const int* pred_labels, const int* gt_labels, int N, int H, int W, int P, int G, const long long* pred_table,
                      int pred_table_rows, const ImThresholds& thr, int T, const ImWs& ws, int* inter, int* pred_rows, int* gt_area,
                      int* match, int* gt_match, int* counts, hipStream_t stream);
