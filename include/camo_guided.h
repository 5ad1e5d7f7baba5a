/* C ABI of the edge-aware mask refinement on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * Stands between the detector's probability map and everything that consumes it.  The region-graph detector paints one probability
 * per superpixel, so its mask is a mosaic whose outline is the SLIC boundary; the GUIDED FILTER (He, Sun, Tang, "Guided Image
 * Filtering") snaps that map to the edges of the image it came from, in closed form: box means, one small solve per pixel, box
 * means again.  camo_guided_filter runs it at the working size with the fp32 image as the guide; camo_guided_apply is the second
 * half of the "fast" variant: it takes the filter's low-resolution coefficients to every image's native size and applies them to
 * the native 8-bit image, so a native-size map gets its edges from the native pixels and not from an interpolated grid.
 * PARITY UNPINNED: the reference has no refinement step and cv2.ximgproc is not part of this package, so the text below is the
 * definition; it is restated in float64 numpy in tests/guided_ref.py, which the kernels are tested against within the rounding of
 * the fp32 outputs (the bounds are in DESIGN.md 10i).
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * check of a pointer or a scalar runs on the host before any launch.  The ABI version is that of camo_fusion.h.  No atomics and no
 * floating-point reduction across threads: every output element is computed by one thread in a fixed order, so two calls give the
 * same bytes, a batch gives the bytes of its images one by one, and the launch count does not depend on N.  Non-finite inputs are
 * the caller's business: they may make any output of their own image non-finite and do nothing else. */
#ifndef CAMO_GUIDED_H
#define CAMO_GUIDED_H
#include <stddef.h>
#include <stdint.h>
#include "camo_resize.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_GF_MAX_RADIUS 64
#define CAMO_GF_MIN_EPS 1e-6        /* below it the one-pass covariance's cancellation is no longer far under the regulariser */
#define CAMO_GF_MAX_EPS 1.0
#define CAMO_GF_FIELDS 4            /* int64 per row of camo_guided_apply's table */

/* Bytes of camo_guided_filter's workspace, (C (C + 1) / 2 + 3 C + 2) doubles per pixel of the batch (136 bytes with a colour guide,
 * 48 with a grey one) and up to 512 bytes of alignment; 0 when the arguments are not supported (the limits below). */
size_t camo_guided_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);

/* The guided filter of an image batch in FOUR launches.
 *   guide  fp32 [N, H, W, C], C = 1 or 3: the image I, values meant in [0, 1].
 *   p      fp32, image i's [H, W] plane at p + i * p_image_stride floats (one channel of a [N, 3, H, W] map is read in place).
 *   radius 1 .. CAMO_GF_MAX_RADIUS; eps CAMO_GF_MIN_EPS .. CAMO_GF_MAX_EPS; clamp 0 or 1.
 *   q      fp32 [N, H, W].   coef  fp32 [N, C + 1, H, W] = abar_0 .. abar_{C-1}, bbar, or null: q is the same either way.
 *   ws     workspace of camo_guided_workspace_bytes(N, H, W, C) bytes, 256-byte aligned.
 * THE WINDOW of pixel k = (y, x) is the pixels within Chebyshev distance `radius` of k that lie INSIDE the image: rows
 * y0 = max(y - r, 0) .. y1 = min(y + r, H - 1), columns x0 = max(x - r, 0) .. x1 = min(x + r, W - 1), cnt = (y1 - y0 + 1)
 * (x1 - x0 + 1) pixels.  Windows are clipped and normalised by their own count, as in the authors' code: nothing is padded and
 * nothing is read across an image's edge.  The window SUM of a plane t is taken separably, in double, in ascending order:
 *   R(y, x) = t(y, x0) + t(y, x0 + 1) + ... + t(y, x1),  S(y, x) = R(y0, x) + R(y0 + 1, x) + ... + R(y1, x),  mean = S / (double)cnt.
 * ARITHMETIC.  Everything between the fp32 inputs and the fp32 outputs is DOUBLE.  The planes summed in the first half are I_c, p,
 * I_c p and I_i I_j (i <= j), each product of two fp32 values formed in double, where it is exact: 4 planes with a grey guide, 13
 * with a colour one.  (The one-pass covariance below cancels: in float it is off by a thousand times the fp32 rounding of the
 * outputs; in double, with eps >= 1e-6 and at most 129^2 terms of magnitude <= 1, the cancellation error is below 1e-9 of a.)
 * With those means, per pixel k:
 *   mu_c = mean(I_c), pbar = mean(p), Sigma_ij = mean(I_i I_j) - mu_i mu_j, c_i = mean(I_i p) - mu_i pbar,
 *   a = (Sigma + eps Id)^-1 c,   b = pbar - sum_c a_c mu_c.
 *   C = 1: a = c / (Sigma + eps).
 *   C = 3: the closed-form inverse of the symmetric matrix M = Sigma + eps Id, adjugate over determinant:
 *          A00 = M11 M22 - M12 M12, A01 = M02 M12 - M01 M22, A02 = M01 M12 - M02 M11, A11 = M00 M22 - M02 M02,
 *          A12 = M01 M02 - M00 M12, A22 = M00 M11 - M01 M01, det = M00 A00 + M01 A01 + M02 A02,
 *          a_0 = (A00 c_0 + A01 c_1 + A02 c_2) / det, a_1 = (A01 c_0 + A11 c_1 + A12 c_2) / det, a_2 = (A02 c_0 + A12 c_1 + A22 c_2) / det.
 * The second half takes the window means abar_c, bbar of the planes a_c, b (kept in double between the halves) over the SAME clipped
 * windows, and q = abar_0 I_0 (+ abar_1 I_1 + abar_2 I_2) + bbar, clamped to [0, 1] when clamp != 0 (fmin(fmax(q, 0), 1)), then
 * converted to fp32 ONCE; coef receives abar_c and bbar converted to fp32 once each (q is formed from the doubles, not from coef).
 * Where two operations may contract into a fused multiply-add is not pinned.
 * Needs 1 <= N <= CAMO_RGD_MAX_IMAGES, H, W in [1, CAMO_RSZ_MAX_SIDE], H * W <= CAMO_RGD_MAX_IMAGE_PIXELS, N * H * W <=
 * CAMO_RGD_MAX_PIXELS, C 1 or 3, radius, eps (not NaN) and clamp in the ranges above, p_image_stride >= H * W, non-null guide, p,
 * q, ws (fp32 pointers 4-byte aligned, ws 256-byte aligned), ws_bytes at least the workspace size: otherwise CAMO_E_ARG.
 * What ws, q and coef hold on entry is unspecified; every element of q, and of coef when it is given, is written.
 *
 * LAUNCHES: row sums of the 4 / 13 planes; their column sums and the solve (a, b to the workspace); row sums of a, b; their column
 * sums and the output.  One thread per pixel in each, 256 threads a block, lanes along a row. */
int camo_guided_filter(const float* guide, const float* p, int64_t p_image_stride, int32_t N, int32_t H, int32_t W, int32_t C,
                       int32_t radius, double eps, int32_t clamp, float* q, float* coef, void* ws, size_t ws_bytes, void* stream);

/* The fast guided filter's second half for a ragged batch in ONE launch: low-resolution coefficients applied to native 8-bit guides.
 *   coef   fp32 [N, C + 1, h, w], camo_guided_filter's (C = 1 or 3).
 *   guide  uint8, guide_elems bytes: image i packed HWC, H_i x W_i x C bytes from guide + guide_off_i (a RaggedImages buffer).
 *   out    fp32, out_elems floats: image i's [H_i, W_i] map from out + out_off_i floats.
 *   table  device memory, int64 [N, CAMO_GF_FIELDS], one row per image:  0 guide_off   1 H_i   2 W_i   3 out_off.
 * PER NATIVE PIXEL (y, x) of image i.  The C + 1 planes of coef[i] are sampled with the BILINEAR rule of camo_resize.h with the whole
 * [h, w] plane as the crop and no flip: per axis n = (2 d + 1) cs - D, i0 = floor(n / (2 D)), w1 = n - i0 2 D, w0 = 2 D - w1, taps
 * clamp(i0, 0, cs - 1) and clamp(i0 + 1, 0, cs - 1) (cs = h, D = H_i for rows; cs = w, D = W_i for columns), den = 4 H_i W_i.  A
 * plane's sample is the sum of (double)(wy wx) (double)value over the four taps in the order (y0, x0), (y0, x1), (y1, x0), (y1, x1),
 * each add rounded once (the products are exact), divided by (double)den and KEPT IN DOUBLE.  Then, in double,
 *   q = a_0 g_0 (+ a_1 g_1 + a_2 g_2) + b,   g_c = (double)u8_c / 255.0,
 * left to right, clamped to [0, 1] when clamp != 0, converted to fp32 once.
 * ROW VALIDITY, as in camo_resize.h: the table is on the device, so the kernel checks every row before it touches memory.  A row is
 * good when H_i and W_i are in [1, CAMO_RSZ_MAX_SIDE], H_i W_i <= max_dst_pixels, both offsets are >= 0, guide_off + H_i W_i C <=
 * guide_elems and out_off + H_i W_i <= out_elems.  A good row gets status[i] = 0.  Any other row gets status[i] = 1 and reads
 * NOTHING; zeros are stored over the elements out_off .. out_off + H_i W_i - 1 that lie inside [0, out_elems) when the destination's
 * own fields (out_off >= 0, the sides, the max_dst_pixels bound) are good, else nothing is stored for it.  status is written with
 * ordinary stores (every block of an image stores the same value).  Rows whose destinations overlap are the caller's business.
 * LAUNCH: grid = (ceil(max_dst_pixels / 1024), N), 256 threads, four pixels a thread in row-major order (lanes along a destination
 * row); the taps are camo_resize's own code and the bytes of an interleaved pixel are fetched as camo_resize fetches them.
 * Needs non-null coef, guide, out, table, status (fp32 pointers and status 4-byte aligned, table 8-byte); 1 <= N <=
 * CAMO_RGD_MAX_IMAGES; C 1 or 3; h, w in [1, CAMO_RSZ_MAX_SIDE], h * w <= CAMO_RGD_MAX_IMAGE_PIXELS, N * h * w <=
 * CAMO_RGD_MAX_PIXELS; guide_elems, out_elems >= 1; 1 <= max_dst_pixels <= CAMO_RGD_MAX_IMAGE_PIXELS; clamp 0 or 1: otherwise
 * CAMO_E_ARG. */
int camo_guided_apply(const float* coef, int32_t N, int32_t C, int32_t h, int32_t w, const uint8_t* guide, int64_t guide_elems,
                      float* out, int64_t out_elems, const int64_t* table, int64_t max_dst_pixels, int32_t clamp,
                      int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
