// Canny edge maps for a batch of images (canny.hip): smoothed Sobel gradients, interpolated non-maximum suppression,
// double threshold, 8-connected hysteresis by union-find.  All launchers return hipError_t as int.
#pragma once
#include "common.h"

constexpr int CANNY_TILE = 32;            // a block's tile is CANNY_TILE x CANNY_TILE pixels of one image
constexpr int CANNY_MAX_RADIUS = 32;      // (tile + 2 + 2 radius)^2 floats of luma plus the two blur stages stay under 64 KB of LDS

struct CannyTaps {
  int radius;                             // int(4 sigma + 0.5)
  float w[2 * CANNY_MAX_RADIUS + 1];      // w[k + radius] = exp(-k^2 / (2 sigma^2)) / sum, k = -radius .. radius
};

struct CannyWs {
  float* grad;             // [N][3][H][W] gi, gj, magnitude (unused when the caller asks for the gradients: they go to its buffer)
  unsigned char* cls;      // [N][H][W] 0 none, 1 weak, 2 strong
  int* label;              // [N][H][W] union-find parent (index into the whole batch), -1 where not weak
  unsigned char* flag;     // [N][H][W] flag[root] = the root's component holds a strong pixel
  size_t bytes;
};
CannyWs canny_carve(size_t npix, void* base);

int launch_canny_gradients(const float* images, int N, int H, int W, const CannyTaps& taps, float* grad, hipStream_t stream);
// grad != null: classes from the gradients (written to ws.cls); grad == null: classes read from cls_in
int launch_canny_hysteresis(const float* grad, const unsigned char* cls_in, float low, float high, int N, int H, int W, const CannyWs& ws,
                            unsigned char* edges, hipStream_t stream);
