/* C ABI of the node targets of the region-graph detector on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * Stands behind the step of the reference's trainer (models/region_graph/train.py, its CODDataset) that turns the ground-truth
 * masks of an image into one target per superpixel for the three node heads: what camo_rg_train.h's camo_rg_loss_backward takes
 * as mask_t, inst_t and edge_t.  The optimizer step that follows the gradients is camo_grad_sumsq + camo_clip_adamw of
 * camo_fusion.h on the flat buffers.
 * PARITY UNPINNED: the reference tree cannot be read here, so neither its majority rule nor its edge rule can be compared.  The
 * text below is the definition; it is restated in numpy (int64) in tests/rg_targets_ref.py, which the kernels are tested against
 * for exact equality.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / negative CAMO_E_* as in
 * camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_RG_TARGETS_H
#define CAMO_RG_TARGETS_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_batch.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_RGTG_TILE 32        /* a block owns a 32 x 32 tile of one image */
#define CAMO_RGTG_TILE_SLOTS 64  /* nodes of a tile that are summed in LDS; a tile with more adds the rest to global memory directly */

/* Targets of every node of a block-diagonal batch of region graphs from ground-truth masks, in THREE launches whatever N is
 * (clear of counts, accumulate over the pixels, finalize over the nodes).  No workspace: `counts` is the accumulator.
 *
 * segments [N, H, W] labels, region_map [N, label_bound] (index of a label within its image or -1), node_off [N + 1]: as
 * camo_rg_region_graph_batch returns them and camo_rg_paint reads them.  gt_mask, gt_instance, gt_edge [N, H, W] uint8; a
 * ground-truth pixel is positive when its byte is > 127.  gt_instance NULL: gt_mask stands in.  gt_edge NULL: the boundary of
 * gt_mask stands in, see below.
 *
 * Which pixels count.  The node of pixel (i, y, x) is v = node_off[i] + region_map[i, s] with s = segments[i, y, x].  The pixel
 * takes part only when 0 <= s < label_bound, region_map[i, s] >= 0 and 0 <= v < n_nodes (the rule of camo_rg_paint); any other
 * pixel adds to no count.
 *
 * counts [n_nodes, 4] int32, per node v over the pixels that take part:
 *   counts[v][0] = pix  its pixels
 *   counts[v][1]        its pixels that are positive in gt_mask
 *   counts[v][2]        its pixels that are positive in gt_instance (in gt_mask when gt_instance is NULL)
 *   counts[v][3]        its edge pixels: positive in gt_edge; with gt_edge NULL, the boundary pixels of gt_mask -- a pixel is
 *                       boundary when it is positive and at least one of its 4-neighbours INSIDE THE IMAGE is not positive (the
 *                       neighbour's byte decides, whether or not the neighbour takes part; the image border itself makes no
 *                       boundary: a mask that covers the whole image has none).
 *
 * Targets, all comparisons in 64-bit integers, band = band_permille, pos = counts[v][1] for mask_t and counts[v][2] for inst_t:
 *   t = 1  when 1000 pos >  (500 + band) pix
 *   t = 0  when 1000 pos <= (500 - band) pix
 *   t = -1 otherwise (the loss ignores the node).
 * band = 0 is strict majority: a tie gives 0 and no node with pixels is ignored.
 *   edge_t[v] = 1.0f when counts[v][3] >= edge_min_pixels, else 0.0f.
 * A node with pix == 0 gets mask_t = inst_t = -1 and edge_t = -1.0f.  Rows v >= n_nodes of the four outputs are not touched.
 * What counts and the three target arrays hold on entry is unspecified; rows 0 .. n_nodes - 1 of all four are written.
 *
 * Every sum is an integer: 32-bit integer LDS atomics per (tile, node), then one 32-bit integer global atomic per (tile, node,
 * non-zero quantity); no floating-point atomic is on the path.  The outputs are functions of the inputs alone: two calls give the
 * same bytes, and a batch gives the rows of its images one by one.
 *
 * Needs N, H, W, label_bound, n_nodes >= 1, label_bound <= CAMO_RG_MAX_LABELS, H * W <= CAMO_RGB_MAX_IMAGE_PIXELS,
 * N * H * W <= CAMO_RGB_MAX_PIXELS, 0 <= band_permille < 500, edge_min_pixels >= 1 and non-null segments, region_map, node_off,
 * gt_mask, counts, mask_t, inst_t, edge_t: otherwise CAMO_E_ARG, and camo_last_error() names the argument. */
int camo_rg_node_targets(const int32_t* segments, const int32_t* region_map, const int32_t* node_off, const uint8_t* gt_mask,
                         const uint8_t* gt_instance, const uint8_t* gt_edge, int32_t N, int32_t H, int32_t W, int32_t label_bound,
                         int32_t n_nodes, int32_t band_permille, int32_t edge_min_pixels, int32_t* counts, int32_t* mask_t,
                         int32_t* inst_t, float* edge_t, void* stream);

#ifdef __cplusplus
}
#endif
#endif
