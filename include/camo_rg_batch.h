/* C ABI of the BATCHED Region-Graph construction on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h
 * (error text: camo_last_error()).  It computes what include/camo_rg_features.h's camo_rg_region_graph computes -- the body of
 * create_region_graph (models/region_graph/extract_rg_embeddings.py:146-236) between its skimage calls -- for N images in one
 * call, as ONE block-diagonal graph ready for camo_rg_node_embeddings, and with order-independent arithmetic.
 * PARITY UNPINNED, as that header says: the checker is oracle/rg_features_oracle.py applied image by image.
 *
 * Arithmetic.  Every per-region sum is an integer sum, so the result is a function of the inputs alone: two calls give the
 * same bytes, and a batch gives the bytes of its images run one by one.  Pixel counts, sum of y, sum of x, edge-map count,
 * perimeter and ring counts are integers already.  Every real quantity q in [0, 1] -- the three channel values, the luma
 * 0.2989 R + 0.5870 G + 0.1140 B and the ring's channel values -- is computed in double from the fp32 pixel exactly as
 * camo_rg_region_graph computes it and added as the integer v = llrint(q * 2^S), S = CAMO_RGB_FIX_BITS = 36, into a 64-bit
 * integer.  The squares are the squares of those integers, v^2 < 2^73, summed exactly in two 64-bit limbs of 36 bits, and a
 * variance is (n sum v^2 - (sum v)^2) / n^2 with the numerator in 128-bit integers.  An image has at most
 * CAMO_RGB_MAX_IMAGE_PIXELS = 2^26 pixels, so every sum and limb stays below 2^63.
 *
 * Unit u = 2^-36 (1.5e-11).  Derived bounds of each feature against exact arithmetic on the same fp32 pixels, BEFORE the one
 * rounding of the result to fp32 (relative 2^-24):
 *   mean R, G, B and the ring means      exact when every value is 0 or >= 2^(23-S) = 2^-13 (its fp32 ulp is then a multiple
 *                                        of u); otherwise each pixel is off by at most u/2, and so is the mean
 *   boundary contrast                    a norm of differences of such means: exact likewise, else <= sqrt(3) u
 *   luma mean                            <= u/2 (luma is a double, rounded once per pixel)
 *   variances (R, G, B, luma)            exact for the fixed-point values v; each v is off by at most u/2 (colours: by 0 under
 *                                        the condition above), which moves a variance by at most 2 std (u/2) + u^2/4 <= u.
 *                                        Stated bound: 3 * 2^-(S+1) = 3 u/2 = 2.2e-11 = CAMO_RGB_VAR_BOUND; feature 14 (luma
 *                                        variance) carries exactly this
 *   std features (3, 4, 5, 7)            |sqrt(a) - sqrt(b)| <= |a - b| / (sqrt(a) + sqrt(b)): <= 1.5 u / std, never more than
 *                                        sqrt(1.5 u) = 4.7e-6; a region of ONE flat colour has variance and std exactly 0
 *   centroid, size, compactness, edge    integer sums: exact
 * Images are expected in [0, 1] as in the reference; a value outside is added all the same and may wrap the sums.
 *
 * Device pointers only, enqueue-only on `stream`, no allocation, no synchronisation, no environment variables;
 * 0 = ok / negative CAMO_E_* as in camo_fusion.h.  Argument checks run on the host before any launch. */
#ifndef CAMO_RG_BATCH_H
#define CAMO_RG_BATCH_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_features.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_RGB_FIX_BITS 36
#define CAMO_RGB_VAR_BOUND 2.18278728425502777e-11           /* 3 * 2^-37 */
#define CAMO_RGB_MAX_IMAGE_PIXELS (1 << 26)                  /* H * W: 2^26 * 2^36 < 2^63 */
#define CAMO_RGB_MAX_PIXELS (1 << 27)                        /* N * H * W: at most 8 directed edges per pixel fit an int32 */
#define CAMO_RGB_MAX_IMAGES 4096
#define CAMO_RGB_TILE_SLOTS 64                               /* labels a 32 x 32 tile sums in LDS; further ones go to global memory */

/* 0 when the arguments are out of range (camo_last_error() says which). */
size_t camo_rg_batch_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t label_bound);

/* images [N, H, W, 3] fp32 in [0, 1]; segments [N, H, W] int32; canny [N, H, W] uint8 (0 / 1); the labels of every image lie in
 * [0, label_bound), 1 <= label_bound <= CAMO_RG_MAX_LABELS.
 * Out, packed over the batch in image order:
 *   x [node_capacity, 15]           rows node_off[n] .. node_off[n + 1] are image n's regions, in increasing label order with
 *                                   empty labels dropped; node_capacity >= N * label_bound is required (it always suffices)
 *   region_map [N, label_bound]     index of the label WITHIN its image, or -1
 *   edge_index [2, edge_capacity]   int64, GLOBAL node indices (block-diagonal), image after image; within an image sorted by
 *                                   (i, j), i < j, each edge followed by its reverse: camo_rg_region_graph's order plus node_off[n]
 *   edge_attr [edge_capacity]
 *   node_off [N + 1], edge_off [N + 1]   int32 prefix sums (edge_off counts directed edges)
 *   batch [node_capacity]           int32 image index of every node (first node_off[N] entries valid)
 *   status [2]                      {pixels whose label lies outside [0, label_bound), directed edges needed = edge_off[N]}
 * A pixel with an out-of-range label is counted in status[0] and otherwise takes no part (as a neighbour neither).  When the
 * batch has more than edge_capacity directed edges, edge_off / status[1] still report what is needed and nothing is written
 * beyond the capacity.  Position features divide by 256 and the size feature by 256^2 whatever H and W are, as the
 * reference does.  Refused: N < 1 or > CAMO_RGB_MAX_IMAGES, H * W > CAMO_RGB_MAX_IMAGE_PIXELS, N * H * W > CAMO_RGB_MAX_PIXELS,
 * label_bound out of range, node_capacity < N * label_bound, edge_capacity < 2, a workspace smaller than the query's.
 * What workspace and the outputs hold on entry is unspecified.  Every element of region_map, node_off, edge_off and status is
 * written, the first node_off[N] rows of x and batch and the first min(edge_off[N], edge_capacity) columns of edge_index and
 * edge_attr; what lies past them is not. */
int camo_rg_region_graph_batch(const float* images, const int32_t* segments, const uint8_t* canny, int32_t N, int32_t H, int32_t W,
                               int32_t label_bound, void* workspace, size_t workspace_bytes, float* x, int32_t node_capacity,
                               int32_t* region_map, int64_t* edge_index, float* edge_attr, int32_t edge_capacity, int32_t* node_off,
                               int32_t* edge_off, int32_t* batch, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
