// Batched region-graph construction (rg_batch.hip): per-region integer sums, bit adjacency, block-diagonal edge list.
// All launchers return hipError_t as int.
#pragma once
#include "common.h"

constexpr int RGB_NACC = 21;      // 64-bit integer sums per (image, label): see rg_batch.hip
constexpr int RGB_SLOTS = 64;     // = CAMO_RGB_TILE_SLOTS
constexpr int RGB_FIX_BITS = 36;  // = CAMO_RGB_FIX_BITS

struct RgBatchWs {
  unsigned long long* acc;  // [N][label_bound][RGB_NACC]      zeroed by the first launch
  unsigned int* adj;        // [N][label_bound][words]         "     bit b of row a, a < b: labels a and b touch under 8-connectivity
  int* kept;                // [N] non-empty labels of each image
  int* rowcount;            // [N][label_bound] neighbours b > a of label a
  int* rowoff;              // [N][label_bound] exclusive prefix of rowcount within the image
  int* pairs;               // [N] undirected edges of each image
  int words;                // adjacency words per row
  size_t bytes;
};
RgBatchWs rg_batch_carve(int N, int label_bound, void* base);

int launch_region_graph_batch(const float* images, const int* segments, const unsigned char* canny, int N, int H, int W, int label_bound,
                              const RgBatchWs& ws, float* x, int* region_map, long long* edge_index, float* edge_attr, int edge_capacity,
                              int* node_off, int* edge_off, int* batch, int* status, hipStream_t stream);
