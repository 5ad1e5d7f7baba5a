/* C ABI of the SLIC superpixel label maps on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * Stands behind the reference's skimage.segmentation.slic(img_u8, n_segments, compactness=10, sigma=1)
 * (models/region_graph/extract_rg_embeddings.py:143-144) with the defaults of scikit-image >= 0.19 that the call leaves alone:
 * max_num_iter=10, convert2lab, enforce_connectivity, min_size_factor=0.5, max_size_factor=3, start_label=1.  The label map is
 * the `segments` input of camo_rg_features.h, for a batch of images, on the device.
 * PARITY UNPINNED: skimage is absent here, its source is not at hand and the reference pins no version of it.  THIS TEXT is the
 * definition of what is computed; tests/slic_ref.py restates it with numpy / scipy.ndimage and the kernels are tested against that.
 *
 *  1 quantise   q = trunc(fp32(x) * 255.0f) (one rounding), clamped to [0, 255]; v = q / 255.  The reference's
 *               (image * 255).astype(np.uint8) followed by img_as_float.
 *  2 smooth     per channel, separable Gaussian with sigma: radius int(4 sigma + 0.5) (9 taps at sigma = 1), weights
 *               exp(-k^2 / (2 sigma^2)) normalised to sum 1, along x then along y, boundary scipy.ndimage's "reflect"
 *               (d c b a | a b c d | d c b a).  sigma == 0 skips the step.
 *  3 Lab        sRGB to linear: v > 0.04045 ? ((v + 0.055) / 1.055)^2.4 : v / 12.92.  XYZ with the rows
 *               (0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227), divided by the
 *               D65 2-degree white (0.95047, 1, 1.08883).  f(t) = t > 0.008856 ? cbrt(t) : 7.787 t + 16 / 116.
 *               L = 116 f(y) - 16, a = 500 (f(x) - f(y)), b = 200 (f(y) - f(z)); all three times 1 / compactness.
 *  4 grid       skimage.util.regular_grid((1, H, W), n_segments): s = sqrt(H W / n_segments) in double,
 *               step = round-half-even(s), start = floor(s / 2); centres at start + i step along both axes while inside the
 *               image: ny = ceil((H - start) / step), nx likewise, k = iy nx + ix, K = ny nx.  A centroid is
 *               (cy, cx, L, a, b); its initial colour is ZERO, as skimage leaves it.
 *               Needs H W > n_segments, min(H, W) >= s and K <= CAMO_RG_MAX_LABELS - 1 (else CAMO_E_UNSUPPORTED).
 *  5 assign     pixel (y, x) is a candidate of centroid k when (int)max(cy - 2 step, 0) <= y < (int)min((cy + 2 step) + 1, H)
 *               and likewise in x.  d = (dy + dx) * w + ((dl^2 + da^2) + db^2) with dy = (cy - y)^2, dx = (cx - x)^2,
 *               w = 1 / step^2: fp32, each operation rounded once, in this order, nothing fused (the window bounds too).
 *               The smallest d wins; equal d goes to the lowest k; a pixel with no candidate gets k = 0 and d = +inf.
 *  6 update     a centroid becomes the mean of (y, x, L, a, b) over the pixels assigned to it; one with no pixel KEEPS its
 *               value (deviation: skimage divides 0 by 0).  The sums are integers, so the result does not depend on the
 *               order of summation: y and x as they are, each colour as the int64 fixed-point number
 *               round-half-even(c * 2^24) (exact for |c| >= 1, absolute error <= 2^-25 below).  The mean is
 *               fp32(double(sum) / double(count)) for y and x and fp32(double(sum) / (double(count) * 2^24)) for the colours.
 *  7 iterate    ten rounds of assign then update; the labels are those of the tenth assign, plus 1.  (The tenth update
 *               cannot change them and is not run.)
 *  8 connect    min_size = int(0.5 (H W / K)), max_size = int(3 (H W / K)) in double.  skimage's sequential relabelling,
 *               stated as a function of the label map: take the 4-connected components of equal labels in raster order of
 *               their first pixel.  A component of at least min_size pixels receives the next new label, starting at 1.  A
 *               smaller one receives `adjacent`: a breadth-first search from the component's first pixel visits the
 *               neighbours of each pixel in the order +x, -x, +y, -y, appends those of the component not yet seen, and sets
 *               `adjacent` to the output label of every neighbour it meets that belongs to a component whose first pixel
 *               comes earlier (such a component is already labelled; a small one carries the label it adopted, 0 included).
 *               The last one met stands.  `adjacent` is 0 when the search meets none, so label 0 can appear in the output;
 *               the reference's loop over regions skips label 0.
 *               Deviation: a component of max_size pixels or more is NOT split (skimage cuts its search there);
 *               counts[n][1] tells how many such components image n had, so a caller can tell.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation; camo_slic is 37 launches whatever N is),
 * 0 = ok / negative CAMO_E_* as in camo_fusion.h.  No floating-point atomics: the same call gives the same bytes, and a batch
 * gives what its images give one by one.  The stage entry points run exactly the kernels that camo_slic runs. */
#ifndef CAMO_SLIC_H
#define CAMO_SLIC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_SLIC_MAX_RADIUS 32            /* int(4 sigma + 0.5) <= 32 */
#define CAMO_SLIC_MAX_IMAGE_PIXELS (1 << 24) /* H * W */
#define CAMO_SLIC_MAX_PIXELS (1 << 30)     /* N * H * W (32-bit pixel indices) */
#define CAMO_SLIC_MAX_IMAGES 65535         /* N */
#define CAMO_SLIC_MIN_COMPACTNESS 0.0625f  /* keeps the int64 colour sums of step 6 below 2^63 */
#define CAMO_SLIC_ITERATIONS 10

/* Step 4 on the host: out[5] = {K, step, start, ny, nx}. */
int camo_slic_grid(int32_t H, int32_t W, int32_t n_segments, int32_t* out);

/* Bytes camo_slic needs; with n_segments == 0 the bytes camo_slic_connect needs (they depend on N, H, W alone).
 * 0 (and an error text) when the shape is out of range or the grid of step 4 is refused. */
size_t camo_slic_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t n_segments);

/* images [N, H, W, 3] fp32 in [0, 1] -> labels [N, H, W] int32 and counts [N, 2] = {largest label + 1, components of max_size
 * pixels or more}.  Needs compactness >= CAMO_SLIC_MIN_COMPACTNESS and sigma >= 0.  What workspace, labels and counts hold on entry
 * is unspecified; every element of labels and counts is written. */
int camo_slic(const float* images, int32_t N, int32_t H, int32_t W, int32_t n_segments, float compactness, float sigma,
              void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* counts, void* stream);

/* Steps 1-3: images [N, H, W, 3] -> lab [N, H, W, 3] fp32 (L, a, b times 1 / compactness).  One launch. */
int camo_slic_preprocess(const float* images, int32_t N, int32_t H, int32_t W, float compactness, float sigma, float* lab,
                         void* stream);

/* Step 5: lab [N, H, W, 3], centroids [N, K, 5] = (cy, cx, L, a, b) -> nearest [N, H, W] in [0, K), dist [N, H, W].  One launch. */
int camo_slic_assign(const float* lab, const float* centroids, int32_t N, int32_t H, int32_t W, int32_t K, int32_t step,
                     int32_t* nearest, float* dist, void* stream);

/* Step 6: centroids [N, K, 5] updated in place from lab and nearest (entries outside [0, K) are ignored).  sums: scratch of
 * N * K * 6 int64.  Three launches (camo_slic clears the sums once and lets each update leave them cleared: two).  What sums hold
 * on entry is unspecified and what they hold on return is not promised; every centroid that has a pixel is written. */
int camo_slic_update(const float* lab, const int32_t* nearest, int32_t N, int32_t H, int32_t W, int32_t K, int64_t* sums,
                     float* centroids, void* stream);

/* Step 8 for any label map: labels_in [N, H, W] -> labels [N, H, W], counts [N, 2] as above.  Needs min_size >= 0, max_size >= 1
 * and a workspace of camo_slic_workspace_bytes(N, H, W, 0).  Seven launches.  What workspace, labels and counts hold on entry is
 * unspecified; every element of labels and counts is written. */
int camo_slic_connect(const int32_t* labels_in, int32_t N, int32_t H, int32_t W, int32_t min_size, int32_t max_size,
                      void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
