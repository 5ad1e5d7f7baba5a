// COCO run-length masks (rle.hip, include/camo_rle.h): what the kernels, the launchers and the entry points share.
// The launchers return hipError_t as int.
#pragma once
#include "common.h"

constexpr int RLE_TILE = 64;             // a tile is RLE_TILE x RLE_TILE pixels; a column segment is RLE_TILE rows of one column

struct RleRunsWs {
  int* seg;                // [N][W][ceil(H / 64)] heads of every column segment, column-major: the order of the positions
  int* pre;                // the same shape: seg's exclusive prefix within the image
  size_t bytes;
};
RleRunsWs rle_runs_carve(int N, int H, int W, void* base);

struct RleDecodeWs {
  int* start;              // [total] the position a count's run starts at, clamped to H W
  size_t bytes;
};
RleDecodeWs rle_decode_carve(int total, void* base);

int launch_rle_runs(const int* labels, int N, int H, int W, int R, const RleRunsWs& ws, int* runs, int* counts, hipStream_t stream);
int launch_rle_decode(const int* cnts, int total, const int* ann_off, const int* ann_image, const int* ann_value, int A, int N, int H, int W,
                      const RleDecodeWs& ws, int* labels, long long* ann_sum, hipStream_t stream);
