// Node targets of the region-graph detector from ground-truth masks (rg_targets.hip, include/camo_rg_targets.h).  The launcher
// returns hipError_t as int; the caller has checked the arguments.
#pragma once
#include "common.h"

constexpr int RGTG_TILE = 32;     // CAMO_RGTG_TILE
constexpr int RGTG_SLOTS = 64;    // CAMO_RGTG_TILE_SLOTS

// three launches: counts [n_nodes, 4] cleared, the pixels added, the targets of the n_nodes rows written
int launch_rg_node_targets(const int* segments, const int* region_map, const int* node_off, const unsigned char* gt_mask,
                           const unsigned char* gt_instance, const unsigned char* gt_edge, int N, int H, int W, int label_bound, int n_nodes,
                           int band_permille, int edge_min_pixels, int* counts, int* mask_t, int* inst_t, float* edge_t, hipStream_t stream);
