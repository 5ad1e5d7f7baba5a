/* C ABI of the camouflaged-object benchmark measures on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * Stands behind the four numbers every camouflaged-object detection table (COD10K, CAMO, NC4K, CHAMELEON) reports next to the mean
 * absolute error: the structure measure S-alpha, the enhanced-alignment measure E-phi (adaptive, mean and maximum over 256
 * thresholds), the F-beta curve (adaptive, mean, maximum) and the weighted F-measure F-beta-w.  All but the last are functions of a
 * small integer table per image -- 256-bin histograms of the 8-bit prediction, split by ground truth and by the S-measure's four
 * quadrants -- which camo_seg_histograms fills; the last needs an exact Euclidean distance transform with nearest-pixel indices,
 * which camo_seg_weighted_f takes.  The device sums integers only, so every output is a function of the inputs alone (two calls
 * give the same bytes, a batch gives the rows of its images one by one); the ratios are taken from the integers in float64 on the
 * host (camouflage_multimodal_amd/seg_measures.py) exactly as written below.
 * PARITY UNPINNED: the reference's utils/metrics.py and the usual evaluation toolkits cannot be read here, so their conventions
 * (epsilons, the treatment of empty masks, the rounding of the centroid, whether a map is min-max normalised first) cannot be
 * compared.  The text below is the definition; it is restated in numpy from the pixel arrays -- without histograms, the distance
 * transform by brute force over all pairs of pixels -- in tests/seg_measures_ref.py, which the kernels and the host ratios are
 * tested against.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / negative CAMO_E_* as in
 * camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h.
 *
 * QUANTISATION, shared by everything below.  A prediction `pred` (fp32) becomes the 8-bit value
 *   q = (int) rintf(fminf(fmaxf(pred, 0.f), 1.f) * 255.0f)
 * -- the multiply in fp32, rounding to nearest with ties to even, a NaN gives 0 -- and p = q / 255 in double wherever a real value
 * is needed.  A ground-truth pixel is positive (g = 1) when gt > 127, else g = 0.  There is NO min-max normalisation of a map: a
 * caller who wants it does it in torch before the call.
 *
 * Below, eps = 2^-52, n = H W, and `a / b` of two integers is ONE correctly rounded float64 division of the exact integers. */
#ifndef CAMO_SEG_MEASURES_H
#define CAMO_SEG_MEASURES_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_detect.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_SEG_BINS 256          /* values of q */
#define CAMO_SEG_QUADRANTS 4
#define CAMO_SEG_HIST_INTS 2048    /* int32 per image of the table: CAMO_SEG_QUADRANTS * 2 * CAMO_SEG_BINS */
#define CAMO_SEG_WF_MAX_SIDE 2048  /* H and W of a weighted-F call */

/* The table of an image batch in THREE launches (a clear, the centroid, the fill; all grids over the whole batch).
 * pred and gt are exactly as for camo_seg_counts: image i's [H, W] plane starts at pred + i * pred_image_stride floats (one channel
 * of a [N, C, H, W] map is read in place), gt [N, H, W] uint8.  Outputs: split int32 [N, 2] = (X, Y) and hist int32
 * [N, CAMO_SEG_QUADRANTS, 2, CAMO_SEG_BINS]; hist must be 8-byte aligned (its rows hold the centroid's 64-bit sums between the
 * second and the third launch).
 *   Split point.  The second launch takes n_fg, Sx, Sy = the number of positive pixels and the sums of their column and row indices
 *   (64-bit integer atomics); the block that finishes an image last computes, in integer arithmetic,
 *     cx = rint(Sx / n_fg), cy = rint(Sy / n_fg)    as exact rationals, a half to the even neighbour,
 *     cx = rint(W / 2),     cy = rint(H / 2)        likewise, when there is no positive pixel,
 *   and X = cx + 1, Y = cy + 1, so 1 <= X <= W and 1 <= Y <= H.
 *   Table.  hist[i, k, g, q] = the number of pixels of image i in quadrant k with ground truth g and quantised value q; the quadrants
 *   are 0 = rows [0, Y) x columns [0, X), 1 = [0, Y) x [X, W), 2 = [Y, H) x [0, X), 3 = [Y, H) x [X, W).  Quadrants 1 to 3 may be empty.
 * Per-wave histograms in LDS, equal consecutive values combined in registers first, the non-zero bins flushed once per block with
 * 32-bit INTEGER atomics: no floating-point atomic is on the path.
 * Needs N >= 1, N <= CAMO_RGD_MAX_IMAGES, H, W >= 1, 2 <= H * W <= CAMO_RGD_MAX_IMAGE_PIXELS (so every count fits int32),
 * pred_image_stride >= H * W: otherwise CAMO_E_ARG.
 * What hist and split hold on entry is unspecified; every element of both is written.
 *
 * The measures are not part of the ABI; the Python surface computes them from the table with these conventions, every decision
 * ("is this sum zero") taken on the exact integers and never on a rounded float.  Per image, with h[g][q] = the table summed over
 * the quadrants, G = sum_q h[1][q] (positive pixels), Q = sum over the pixels of q:
 *   MAE8 = (sum over the pixels of |q - 255 g|) / (255 n).
 *   Binarisation at t = 0..255: predicted positive when q >= t.  TP, FP, FN, TN as usual, Pn = TP + FP.
 *   Adaptive binarisation: p >= min(2 mean(p), 1), decided in integers as q n >= min(2 Q, 255 n); it is the binarisation at
 *     t_a = ceil(min(2 Q, 255 n) / n).
 *   F-beta, beta^2 = 0.3: P = TP / Pn (1 when Pn = 0), R = TP / G (1 when G = 0), F = 1.3 P R / (0.3 P + R), and F = 0 when the
 *     numerator is 0 (TP = 0 and Pn + G > 0).  f_curve[t] = F at t; f_max and f_mean = the maximum and the mean (the sum in increasing
 *     t, divided by 256) of the curve; f_adp = F at t_a, and 0 when its TP is 0.
 *   E-phi of a binarisation:  G = 0: (n - Pn) / (n - 1 + eps);  G = n: Pn / (n - 1 + eps);  otherwise with mp = Pn / n, mg = G / n and
 *     phi(a, b) = (2 a b / (a a + b b + eps) + 1)^2 / 4:
 *     E = [TP phi(1 - mp, 1 - mg) + FP phi(1 - mp, -mg) + FN phi(-mp, 1 - mg) + TN phi(-mp, -mg)] / (n - 1 + eps), summed left to right.
 *     e_curve, e_max, e_mean, e_adp as for F (e_adp has no special case).
 *   S-alpha, alpha = 0.5, u = G / n:  G = 0: 1 - Q / (255 n);  G = n: Q / (255 n);  otherwise S = max(0, 0.5 S_o + 0.5 S_r).
 *     S_o = u o_fg + (1 - u) o_bg with o = 2 x / (x x + 1 + sigma + eps), where for a class of c pixels with q-sum s and q^2-sum s2:
 *       x = s / (255 c) for the positive class (the mean of p) and (255 c - s) / (255 c) for the background class (the mean of 1 - p),
 *       sigma = sqrt((c s2 - s s) / (65025 c (c - 1))), the sample standard deviation (ddof 1), and 0 when c = 1.
 *     S_r = sum over the non-empty quadrants of w ssim, w = m / n for a quadrant of m pixels with q-sum s, q^2-sum s2, Gk positive
 *       pixels and q-sum s1 over them:  x = s / (255 m), y = Gk / m,
 *       sx = ((m s2 - s s) / (65025 m)) / (m - 1 + eps), sy = ((m Gk - Gk Gk) / m) / (m - 1 + eps),
 *       sxy = ((m s1 - s Gk) / (255 m)) / (m - 1 + eps),  a = 4 x y sxy,  b = (x x + y y)(sx + sy),
 *       ssim = a / (b + eps) when a != 0 (s, Gk and m s1 - s Gk all non-zero); 1 when a = 0 and b = 0 (s = Gk = 0, or m s2 = s s and
 *       m Gk = Gk Gk); else 0. */
int camo_seg_histograms(const float* pred, int64_t pred_image_stride, const uint8_t* gt, int32_t N, int32_t H, int32_t W, int32_t* hist,
                        int32_t* split, void* stream);

/* Bytes of camo_seg_weighted_f's workspace; 0 when the arguments are not supported. */
size_t camo_seg_weighted_f_workspace_bytes(int32_t N, int32_t H, int32_t W);

/* The sums behind the weighted F-measure, per image, in FOUR launches (a clear, the distance transform's column pass and row pass,
 * the weighting; all grids over the whole batch).  pred, pred_image_stride, gt as above; gauss: 49 doubles on the device, the 7 x 7
 * kernel exp(-(dx^2 + dy^2) / (2 * 5^2)), dx, dy = -3..3, row-major in (dy, dx), divided by its sum (the caller computes it once on
 * the host, so the device and a reference use the same bytes); ws: workspace of camo_seg_weighted_f_workspace_bytes(N, H, W) bytes,
 * 256-byte aligned.  Output sums int64 [N, 3] = (n_fg, A_fg, A_bg).  Per image, E = |p - g| in double:
 *   1. Exact squared Euclidean distance transform with indices: every background pixel (y, x) gets the positive pixel (y', x') of
 *      least integer d2 = (y - y')^2 + (x - x')^2, ties to the smaller (y', x') in row-major order.  (Column pass: the nearest
 *      positive row of every column by scan, a tie to the smaller y'; row pass: the minimum of (x - x')^2 + dy(y, x')^2 over x'.)
 *   2. Et = E on a positive pixel and E of the nearest positive pixel on a background one.
 *   3. EA = the 7 x 7 correlation of Et with gauss, EA[y, x] = sum_{j, i} gauss[j, i] Et[y + j - 3, x + i - 3] (taps in row-major order,
 *      zero outside the image), in double.
 *   4. m = min(E, EA) on a positive pixel, E on a background one.
 *   5. B = 1 on a positive pixel, 2 - exp(ln(0.5) / 5 * sqrt(d2)) on a background one.
 *   6. n_fg = the number of positive pixels; A_fg and A_bg = the sums over the positive and over the background pixels of
 *      llrint(m B 2^32), by 64-bit INTEGER atomics after block-level sums.
 *   An image with no positive pixel gets (0, 0, 0): it has no nearest pixel and none is dereferenced.
 * The double exp and sqrt are the device's, so A_fg and A_bg agree with a host restatement to about one unit of 2^-32 per pixel.
 * The host ratio, with a = A / 2^32: TPw = n_fg - a_fg, R = 1 - a_fg / n_fg, P = TPw / (TPw + a_bg + eps),
 *   F-beta-w = 2 R P / (R + P + eps), and 0 when n_fg = 0.
 * Needs N >= 1, N <= CAMO_RGD_MAX_IMAGES, 1 <= H, W <= CAMO_SEG_WF_MAX_SIDE, H * W >= 2, pred_image_stride >= H * W, ws_bytes at
 * least the workspace size: otherwise CAMO_E_ARG.  What ws and sums hold on entry is unspecified; every element of sums is written. */
int camo_seg_weighted_f(const float* pred, int64_t pred_image_stride, const uint8_t* gt, int32_t N, int32_t H, int32_t W,
                        const double* gauss, void* ws, size_t ws_bytes, int64_t* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif
