/* C ABI of the Canny edge maps on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h
 * (error text: camo_last_error()).
 *
 * Stands behind the reference's skimage.feature.canny(gray, sigma=2) (models/region_graph/extract_rg_embeddings.py:151-152):
 * the edge map that the region-graph construction of camo_rg_features.h takes as an input, for a batch of images, on the device.
 * PARITY UNPINNED: skimage is absent here and the reference pins no version of it.  What is computed is the published
 * scikit-image algorithm with the reference's arguments, restated below and, with scipy.ndimage, in tests/canny_ref.py,
 * which these kernels are tested against.
 *
 *  1 luma       0.2989 r + 0.5870 g + 0.1140 b
 *  2 smoothing  separable Gaussian of radius int(4 sigma + 0.5), weights normalised to sum 1, zero outside the image; the
 *               result is divided by the same blur of an all-ones image (+ 2^-52)
 *  3 gradients  3 x 3 Sobel with scipy.ndimage.sobel's scaling (smoothing 1 2 1, difference -1 0 1, no division), the border
 *               pixel repeated: gi along rows (down), gj along columns (right), m = sqrt(gi^2 + gj^2)
 *  4 classes    interior pixels only (the one-pixel border of the image never carries an edge).  s = +1 when gi and gj have
 *               the same sign or either is zero, else -1.
 *                 |gi| >= |gj|: a = |gj|, b = |gi|, forward pair c1 = m[r+1, c], c2 = m[r+1, c+s], backward c1 = m[r-1, c], c2 = m[r-1, c-s]
 *                 otherwise   : a = |gi|, b = |gj|, forward pair c1 = m[r, c+s], c2 = m[r+1, c+s], backward c1 = m[r, c-s], c2 = m[r-1, c-s]
 *               local maximum: c2 * a + c1 * (b - a) <= m * b for both pairs (scikit-image's bilinear test times b: ties kept),
 *               in fp32, each operation rounded once, in this order, nothing fused.  weak: local maximum and m >= low;
 *               strong: local maximum and m >= high.
 *  5 hysteresis a weak pixel is an edge exactly when its 8-connected component of weak pixels contains a strong one.
 *
 * Device pointers only, enqueue-only on `stream` (five launches for camo_canny, four for camo_canny_hysteresis, no
 * allocation, no synchronisation), 0 = ok / negative CAMO_E_* as in camo_fusion.h.  The result does not depend on scheduling. */
#ifndef CAMO_CANNY_H
#define CAMO_CANNY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_CANNY_MAX_RADIUS 32          /* int(4 sigma + 0.5) <= 32 */
#define CAMO_CANNY_MAX_PIXELS (1 << 30)   /* N * H * W */

/* 0 (and an error text) when N, H or W is < 1 or N * H * W exceeds CAMO_CANNY_MAX_PIXELS */
size_t camo_canny_workspace_bytes(int32_t N, int32_t H, int32_t W);

/* images [N, H, W, 3] fp32 in [0, 1] -> edges [N, H, W] (0 / 1); grad, when not NULL, receives [N, 3, H, W] = gi, gj, m.
 * Needs N, H, W >= 1, sigma > 0, 0 < low <= high.  What workspace, edges and grad hold on entry is unspecified; every element of
 * edges, and of grad when it is given, is written. */
int camo_canny(const float* images, int32_t N, int32_t H, int32_t W, float sigma, float low, float high, void* workspace,
               size_t workspace_bytes, uint8_t* edges, float* grad, void* stream);

/* Step 5 alone, as camo_canny runs it: cls [N, H, W] with 0 none, 1 weak, 2 strong -> edges [N, H, W] (0 / 1).  Same workspace.
 * What workspace and edges hold on entry is unspecified; every element of edges is written. */
int camo_canny_hysteresis(const uint8_t* cls, int32_t N, int32_t H, int32_t W, void* workspace, size_t workspace_bytes,
                          uint8_t* edges, void* stream);

#ifdef __cplusplus
}
#endif
#endif
