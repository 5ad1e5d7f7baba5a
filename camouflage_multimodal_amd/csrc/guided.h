// Edge-aware mask refinement (guided.hip, include/camo_guided.h): what the kernels, the launchers and the entry points
// share.  The launchers return hipError_t as int.
#pragma once
#include "common.h"

constexpr int GF_NT = 256;         // threads per block of every kernel here; lanes run along a row
constexpr int GF_APPLY_PIX = 4;    // native pixels per thread of the apply kernel, GF_NT apart in row-major order (resize.hip's span)

constexpr int gf_sum_planes(int C) { return C * (C + 1) / 2 + 2 * C + 1; }      // I_c, p, I_c p, I_i I_j (i <= j): 4 or 13

struct GfWs {
  double* sums;      // [N][gf_sum_planes(C)][H][W] row sums of the first half; then [N][C + 1][H][W] row sums of a, b (the same memory)
  double* ab;        // [N][C + 1][H][W] a_0 .. a_{C-1}, b of every pixel
  size_t bytes;
};
GfWs gf_carve(int N, int H, int W, int C, void* base);

int launch_guided_filter(const float* guide, const float* p, long long p_stride, int N, int H, int W, int C, int radius, double eps, bool clamp,
                         float* q, float* coef, const GfWs& ws, hipStream_t stream);
int launch_guided_apply(const float* coef, int N, int C, int h, int w, const unsigned char* guide, long long guide_elems, float* out,
                        long long out_elems, const long long* table, long long max_dst_pixels, bool clamp, int* status, hipStream_t stream);
