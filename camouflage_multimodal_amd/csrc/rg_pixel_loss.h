// Node weights of the structure loss on the painted mask (rg_pixel_loss.hip, include/camo_rg_pixel_loss.h).  The
// launcher returns hipError_t as int; the caller has checked the arguments.  (The loss itself is rg_train.hip's launch_rgt_pixel_loss.)
#pragma once
#include "common.h"

constexpr int RGPL_MAX_RADIUS = 31;   // CAMO_RGPL_MAX_RADIUS
constexpr int RGPL_MAX_GAIN = 16;     // CAMO_RGPL_MAX_GAIN

// two launches: node_w [n_nodes, 2] cleared, then q and q g of every pixel that takes part added to its node
int launch_rg_pixel_weights(const int* segments, const int* region_map, const int* node_off, const unsigned char* gt_mask, int N, int H, int W,
                            int label_bound, int n_nodes, int radius, int gain, long long* node_w, hipStream_t stream);
