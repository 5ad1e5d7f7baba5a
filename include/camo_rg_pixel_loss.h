/* C ABI of the structure loss on the painted mask of the region-graph detector on MI355X, exported by the same
 * libcamo_fusion.so as include/camo_fusion.h (error text: camo_last_error()).
 *
 * The detector paints one value per superpixel and is judged on pixels (camo_rg_detect.h, camo_seg_measures.h); the loss of
 * camo_rg_train.h trains the mask head on one majority target per node.  This header adds the F3Net "structure loss" (Wei, Wang,
 * Huang: F3Net, AAAI 2020) -- a boundary-weighted binary cross-entropy plus a boundary-weighted soft IoU -- taken on the PAINTED map
 * against the ground-truth mask.  The painted map is constant on a superpixel, so the sums over pixels collapse exactly into two
 * integer weights per node and a reduction over the nodes of an image; no pixel is touched during training.
 * PARITY UNPINNED: the reference tree's trainer (models/region_graph/train.py) cannot be read here and has no pixel loss that is known; the text
 * below is the definition.  It is restated in tests/rg_pixel_loss_ref.py twice, pixel by pixel through the paint and in the node
 * form, and the kernels are tested against both.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / negative CAMO_E_* as in
 * camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_RG_PIXEL_LOSS_H
#define CAMO_RG_PIXEL_LOSS_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_targets.h"
#include "camo_rg_train_drop.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_RGPL_MAX_RADIUS 31 /* the window is (2 radius + 1)^2 <= 63 x 63 */
#define CAMO_RGPL_MAX_GAIN 16   /* F3Net's is 5 */

/* The two integer weights of every node of a block-diagonal batch of region graphs, in TWO launches whatever N is (clear of
 * node_w, accumulate over the pixels).  No workspace: `node_w` is the accumulator.
 *
 * segments, region_map, node_off, gt_mask, N, H, W, label_bound, n_nodes: as camo_rg_node_targets takes them.  Per image i and
 * pixel p = (y, x):
 *   g(p) = 1 when the byte of gt_mask is > 127, else 0
 *   r = radius, K = (2 r + 1)^2
 *   S(p) = the sum of g over the (2 r + 1) x (2 r + 1) window centred on p, clipped to the image (zero padding; the divisor of the
 *          mean is always K: K avg_pool2d(g, 2 r + 1, stride 1, padding r) of torch)
 *   q(p) = K + gain |S(p) - K g(p)|          (K times F3Net's weit = 1 + gain |avg_pool(g) - g|, as an integer)
 * A pixel takes part under the rule of camo_rg_node_targets: 0 <= s < label_bound for its label s, region_map[i, s] >= 0 and
 * 0 <= v < n_nodes for its node v = node_off[i] + region_map[i, s].  A pixel that takes no part adds to no node; its byte still
 * counts in the windows of its neighbours.
 *
 * node_w [n_nodes, 2] int64, per node v over the pixels that take part:
 *   node_w[v][0] = A_v = sum q(p)          node_w[v][1] = B_v = sum q(p) g(p)
 * A node without pixels gets (0, 0).  Rows 0 .. n_nodes - 1 are written, whatever node_w holds on entry; rows past them are not
 * touched.  With radius 0 (K = 1, q = 1) A_v and B_v are columns 0 and 1 of camo_rg_node_targets' counts.
 *
 * Every sum is an integer: 32-bit integer LDS atomics per (tile, node) -- a tile's sum is at most 1024 * 17 * 63^2 < 2^32 -- then
 * one 64-bit integer global atomic per (tile, node, non-zero quantity); no floating-point atomic is on the path.  Two calls give
 * the same bytes, and a batch gives the rows of its images one by one.
 *
 * Needs N, H, W, label_bound, n_nodes >= 1, label_bound <= CAMO_RG_MAX_LABELS, H * W <= CAMO_RGB_MAX_IMAGE_PIXELS,
 * N * H * W <= CAMO_RGB_MAX_PIXELS, 0 <= radius <= CAMO_RGPL_MAX_RADIUS, 0 <= gain <= CAMO_RGPL_MAX_GAIN and non-null segments,
 * region_map, node_off, gt_mask, node_w: otherwise CAMO_E_ARG, and camo_last_error() names the argument. */
int camo_rg_pixel_weights(const int32_t* segments, const int32_t* region_map, const int32_t* node_off, const uint8_t* gt_mask, int32_t N,
                          int32_t H, int32_t W, int32_t label_bound, int32_t n_nodes, int32_t radius, int32_t gain, int64_t* node_w,
                          void* stream);

/* camo_rg_loss_backward_drop (camo_rg_train_drop.h: either batch-norm mode, with or without dropout) with the pixel term added to
 * the loss.  Every argument up to `seed` is that call's and means what it means there; the workspace is that of
 * camo_rg_train_drop_workspace_bytes.  The three existing terms, their targets and their weights are untouched; w_mask = 0 trains
 * the mask head on pixels alone.
 *
 * node_w [N, 2] from camo_rg_pixel_weights with `radius` (row v of node_w is row v of the graph), node_off [n_images + 1] the first
 * node of every image.  node_off is not read on the host: every entry is clamped to [0, N] on the device and a decreasing pair is
 * an empty image, so no content of it makes the call read or write outside its arrays.  (Images that share a node are the caller's
 * mistake: the node's gradient is then unspecified.)
 *
 * Needs num_classes == 2.  Per node v, in fp32, with l = the mask head's two logits:
 *   z_v = l[v][1] - l[v][0]        p_v = 1 / (1 + expf(-z_v))        sp(z) = max(z, 0) + logf(1 + expf(-|z|))
 * Per image i, over its nodes v = node_off[i] .. node_off[i + 1] - 1, in double and in a fixed order, K = (2 radius + 1)^2:
 *   SA_i = sum A_v     SB_i = sum B_v     I_i = sum p_v B_v     U_i = sum p_v A_v + SB_i     D_i = U_i - I_i + K
 *   wbce_i = sum [B_v sp(-z_v) + (A_v - B_v) sp(z_v)] / SA_i          wiou_i = 1 - (I_i + K) / D_i
 * which are F3Net's weighted BCE and weighted IoU of the painted map sigmoid(z) of image i (its "+ 1" is K here, A and B being K
 * times its weights).  An image with SA_i = 0 is left out; n_img is the number of images that are left.  The pixel term is
 *   P = sum_i (wbce_i + wiou_i) / n_img,   0 with zero gradient when n_img = 0
 *   dP/dz_v = [ (A_v p_v - B_v) / SA_i - p_v (1 - p_v) (B_v D_i - (I_i + K) (A_v - B_v)) / D_i^2 ] / n_img
 * t_v = w_pixel dP/dz_v is taken in double and rounded to fp32 once; t_v is ADDED to the gradient of l[v][1] and subtracted from
 * that of l[v][0] after the existing terms have written them, and the backward goes on from there as before.
 *
 * loss [6] = total (camo_rg_loss_backward_drop's total + w_pixel P), mask, instance, edge (those three as before), the mean of
 * wbce_i and the mean of wiou_i over the n_img images.  With w_pixel = 0 the first four figures and every gradient are the bytes
 * camo_rg_loss_backward_drop gives.  No floating-point atomic: two calls on the same arrays give the same bytes.
 *
 * Needs what camo_rg_loss_backward_drop needs, num_classes == 2 (CAMO_E_UNSUPPORTED), n_images >= 1, 0 <= radius <=
 * CAMO_RGPL_MAX_RADIUS, w_pixel finite and >= 0, non-null node_w and node_off (CAMO_E_ARG; camo_last_error() names the argument). */
int camo_rg_loss_backward_pixel(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                                const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                                const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                                const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                                float* loss, float* const* grads, float momentum, float* const* running, float* batch_stats,
                                int32_t batch_stats_mode, float p_conv, float p_shared, float p_head, uint64_t seed, const int64_t* node_w,
                                const int32_t* node_off, int32_t n_images, int32_t radius, float w_pixel, void* stream);

#ifdef __cplusplus
}
#endif
#endif
