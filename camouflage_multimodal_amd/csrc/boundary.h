// Boundary IoU (boundary.hip, include/camo_boundary.h): what the kernels, the launchers and the entry points share.
// The launchers return hipError_t as int.
#pragma once
#include "common.h"
#include "inst_match.h"

constexpr int BD_NT = 256;         // threads per block of the two erosion kernels
constexpr int BD_STRIP = 64;       // rows of one image a block of the column pass takes (CAMO_BD_STRIP): one bit each in a 64-bit mask

// rowok: [N][H][W] bytes, the row pass's result
int launch_boundary_labels(const int* labels, int N, int H, int W, int d, int* out, unsigned char* rowok, hipStream_t stream);

struct BdWs {
  int* area_p;             // [N][P + 1] row sums of inter
  int* area_g;             // [N][G + 1] column sums of inter
  int* rank;               // [N][P] 0-based rank of predicted id p (at p - 1) in score order
  int* bd_area_p;          // [N][P + 1] row sums of inter_bd
  int* bd_area_g;          // [N][G + 1] column sums of inter_bd
  int* bd_counts;          // [N][CAMO_IM_COUNTS] the boundary maps' out-of-range pixels: counted, not reported
  size_t bytes;
};
BdWs bd_carve(int N, int P, int G, void* base);

int launch_boundary_match(const int* pred_labels, const int* gt_labels, const int* pred_bd, const int* gt_bd, int N, int H, int W, int P, int G,
                          const long long* pred_table, int pred_table_rows, const ImThresholds& thr, int T, const BdWs& ws, int* inter,
                          int* inter_bd, int* pred_rows, int* gt_area, int* match, int* gt_match, int* counts, hipStream_t stream);
