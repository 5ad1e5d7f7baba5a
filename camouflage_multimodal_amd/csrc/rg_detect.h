// Region-graph detector (rg_detect.hip, include/camo_rg_detect.h): the node-classification heads with their probabilities, the
// paint of a per-region value onto the pixels, and the counts of a predicted map against a ground-truth mask.  All launchers
// return hipError_t as int; the callers have checked the arguments.
#pragma once
#include "common.h"

constexpr int RGD_ROWS = 16;        // node rows per block of the heads kernel at hidden <= 256
constexpr int RGD_ROWS_WIDE = 8;    // ... above that: the hidden activations of a tile, [rows][3 hidden / 2] floats, stay under 24 KB of LDS
constexpr int RGD_WIDE_ABOVE = 256;

struct RgdHeads { const float* p[12]; };   // CAMO_RGD_* order

// one launch: logits [n, 2 nc + 1], probs [n, 3] from emb [n, hidden]
int launch_rgd_heads(const RgdHeads& P, const float* emb, int n, int hidden, int nc, float* logits, float* probs, hipStream_t stream);
// one launch: maps [N, C, H, W]
int launch_rgd_paint(const float* values, int n_nodes, int C, const int* segments, const int* region_map, const int* node_off, int N, int H,
                     int W, int label_bound, float fill, float* maps, hipStream_t stream);
// two launches: counts [N, 5] cleared, then TP, FP, FN, TN, A added
int launch_rgd_counts(const float* pred, long long stride, const unsigned char* gt, float threshold, int N, int H, int W,
                      unsigned long long* counts, hipStream_t stream);
