/* C ABI of the Region-Graph construction on MI355X ("next" row 4), exported by the same libcamo_fusion.so
 * as include/camo_fusion.h (error text: camo_last_error()).
 *
 * Stands behind the body of create_region_graph (models/region_graph/extract_rg_embeddings.py:138-246) BETWEEN its three
 * skimage calls: given the image, the superpixel label map `segments` (slic, :144) and the boolean edge map (canny,
 * :152), it produces what the function returns -- node features x [n, 15] (:154-228), edge_index, edge weights
 * (:219-236; the RAG's edge set = pairs of labels that touch under 8-connectivity) -- on the device, ready for
 * the embedding call of camo_rg_gnn.h.  The reference does this in an O(regions x pixels) numpy loop, ~2 s per image.
 * PARITY UNPINNED: skimage is absent here and the reference ships no region-graph fixture; the arithmetic between the
 * skimage calls is restated in oracle/rg_features_oracle.py (with the reference's own scipy.ndimage calls), which these
 * kernels are tested against.  slic and canny themselves stay the caller's.
 *
 * Regions are renumbered in increasing label order, empty labels dropped (the reference's region_id_map); edges come
 * sorted by (i, j), i < j, each followed by its reverse (the reference's order is networkx's: a permutation).
 *
 * Arithmetic of the variance and std features (3, 4, 5, 7, 14).  A region of n pixels has the sums S1 = sum v and S2 = sum v^2 of
 * its values v in [0, 1], added in double by atomics in the order the pixels arrive, and the feature is S2/n - (S1/n)^2, negative
 * results set to 0.  With u = 2^-53 and terms that are all >= 0, n additions in ANY order leave S1 off by at most (n-1) u S1, and
 * S2 -- whose terms carry one rounding of their own -- by at most n u S2.  1/n and the product with it round once each: q = S2/n
 * is off by at most (n+2) u q, the mean m by (n+1) u m and its rounded square by (2n+3) u m^2; the subtraction adds u |var|.
 * With q <= 1 and m^2 <= q,
 *   |var - exact var|  <=  ((n+2) + (2n+3) + 1) u  =  3 (n+2) u  <=  CAMO_RG_VAR_BOUND_PER_PIXEL * n,  9 * 2^-53 per pixel
 * (9 at n = 1; the factor tends to 3), whether or not the compiler contracts the subtraction into an fma (one rounding less).
 * The sign of the error is an accident of the order.  Since |sqrt(a) - sqrt(b)| <= sqrt|a - b|, a std feature is off by at most
 * sqrt(CAMO_RG_VAR_BOUND_PER_PIXEL * n) -- all of it where the exact variance is 0: 3.2e-8 for one pixel, 8.1e-6 for a flat
 * region of 256 x 256 pixels -- and by about (bound) / (2 std) where it is not.  Both are before the one rounding to fp32.
 * camo_rg_region_graph_batch (include/camo_rg_batch.h) sums integers instead and gives a flat region exactly 0.
 *
 * Device pointers only, enqueue-only on `stream`, 0 = ok / negative CAMO_E_* as in camo_fusion.h. */
#ifndef CAMO_RG_FEATURES_H
#define CAMO_RG_FEATURES_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_RG_NFEAT 15
#define CAMO_RG_MAX_LABELS 4096
#define CAMO_RG_VAR_BOUND_PER_PIXEL 9.99200722162640886e-16    /* 9 * 2^-53 */

size_t camo_rg_graph_workspace_bytes(int32_t n_labels);

/* image [H, W, 3] fp32 in [0, 1]; segments [H, W] int32 labels in [0, n_labels); canny [H, W] uint8 (0 / 1).
 * Out: x [n_labels, 15] (first counts[0] rows valid), region_map [n_labels] (new index or -1),
 * edge_index [2, edge_capacity] int64 (row 0 sources, row 1 targets; first counts[1] columns valid), edge_attr
 * [edge_capacity], counts [2] = {regions kept, directed edges}.  When the graph has more than edge_capacity directed
 * edges, counts[1] still reports the number needed and nothing is written beyond the capacity.  The position features
 * divide by 256 and the size feature by 256^2 whatever H and W are, as the reference does (its images are 256 x 256).
 * What workspace and the outputs hold on entry is unspecified.  Every element of region_map and counts is written, the first
 * counts[0] rows of x and the first min(counts[1], edge_capacity) columns of edge_index and edge_attr; what lies past them is not. */
int camo_rg_region_graph(const float* image, const int32_t* segments, const uint8_t* canny, int32_t H, int32_t W,
                         int32_t n_labels, void* workspace, size_t workspace_bytes, float* x, int32_t* region_map,
                         int64_t* edge_index, float* edge_attr, int32_t edge_capacity, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
