/* C ABI of the region-graph detector on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h
 * (error text: camo_last_error()).
 *
 * Stands behind the reference's region-graph-only detector (models/region_graph/test.py::detect_camouflage), the one place of the
 * reference that says WHERE the object is: the node-classification heads of RegionGraphGNN give a mask, an instance and an edge
 * probability per superpixel, each probability is painted onto the superpixel's pixels through the SLIC label map, and the
 * painted mask is scored against a ground-truth mask (IoU, Dice, precision, recall, F1, accuracy, MAE).
 * PARITY UNPINNED: the reference tree, torch_geometric and scikit-image are absent here and no region-graph checkpoint ships, so
 * neither the heads' inputs nor the label maps nor the reference's metric conventions (utils/metrics.py, which cannot be read
 * here: its epsilon convention for empty masks is unknown) can be compared.  The text below is the definition; it is restated in
 * numpy (float64 on the fp32 inputs) in tests/rg_detect_ref.py, which the kernels are tested against.
 *
 * Device pointers only, fp32, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / negative CAMO_E_* as in
 * camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_RG_DETECT_H
#define CAMO_RG_DETECT_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_gnn.h"
#ifdef __cplusplus
extern "C" {
#endif

/* head parameter table: device pointers in this order (state_dict order of the reference module) */
enum {
  CAMO_RGD_MASK_W1 = 0, /* fc_mask_1.weight [hidden/2, hidden] */
  CAMO_RGD_MASK_B1,     /* fc_mask_1.bias [hidden/2] */
  CAMO_RGD_MASK_W2,     /* fc_mask_2.weight [num_classes, hidden/2] */
  CAMO_RGD_MASK_B2,     /* fc_mask_2.bias [num_classes] */
  CAMO_RGD_INST_W1,     /* fc_instance_1.weight, .bias, fc_instance_2.weight, .bias: shapes as for the mask head */
  CAMO_RGD_INST_B1,
  CAMO_RGD_INST_W2,
  CAMO_RGD_INST_B2,
  CAMO_RGD_EDGE_W1,     /* fc_edge_1.weight [hidden/2, hidden] */
  CAMO_RGD_EDGE_B1,     /* fc_edge_1.bias [hidden/2] */
  CAMO_RGD_EDGE_W2,     /* fc_edge_2.weight [1, hidden/2] */
  CAMO_RGD_EDGE_B2,     /* fc_edge_2.bias [1] */
  CAMO_RGD_NPARAMS
};

#define CAMO_RGD_MAX_HIDDEN 512
#define CAMO_RGD_MAX_CLASSES 8
#define CAMO_RGD_MAX_CHANNELS 16
#define CAMO_RGD_MAX_PIXELS (1 << 30)        /* N * H * W of a paint call */
#define CAMO_RGD_MAX_IMAGES 65535            /* N of a counts call */
#define CAMO_RGD_MAX_IMAGE_PIXELS (1 << 26)  /* H * W of a counts call: the absolute-error sum stays below 2^58 */
#define CAMO_RGD_FIX_BITS 32                 /* the absolute error of a pixel is added as llrint(|pred - g| * 2^32) */

/* The three node-classification heads and their probabilities in ONE launch.  emb [n, hidden] is the output of the node-embedding
 * entry point of camo_rg_gnn.h (after fc_shared + ReLU).  Per node with embedding e and per head h in {mask, instance, edge}:
 *   z_h = relu(W1_h e + b1_h)     l_h = W2_h z_h + b2_h       (the dropout layers between them are the identity: eval mode)
 * logits [n, 2 num_classes + 1] = l_mask | l_instance | l_edge, in this column order;
 * probs  [n, 3] = softmax(l_mask)[1], softmax(l_instance)[1], sigmoid(l_edge).
 * Exact fp32: every product is an fmaf into an fp32 sum (first layer: one sum per output in increasing input order; second layer:
 * 64 partial sums of stride 64 added in a fixed tree); the exponentials are the device's fast ones.  The result is a function of
 * the inputs alone.  dims->in_channels and dims->heads are not used.
 * Needs n >= 1, 2 <= hidden <= CAMO_RGD_MAX_HIDDEN and even, 2 <= num_classes <= CAMO_RGD_MAX_CLASSES: otherwise CAMO_E_ARG. */
int camo_rg_node_heads(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* head_params, const float* emb, int32_t n,
                       float* logits, float* probs, void* stream);

/* A value per region painted onto the region's pixels, for a batch, in ONE launch: values [n_nodes, C] rows of the block-diagonal
 * graph, segments [N, H, W] labels, region_map [N, label_bound] (index of a label within its image or -1), node_off [N + 1] ->
 * maps [N, C, H, W]:
 *   maps[i, c, y, x] = values[node_off[i] + region_map[i, s], c]   with s = segments[i, y, x],
 * when 0 <= s < label_bound, region_map[i, s] >= 0 and the row index is below n_nodes; otherwise `fill`.  A pure gather: bit-exact.
 * Needs 1 <= C <= CAMO_RGD_MAX_CHANNELS, n_nodes >= 1, N, H, W, label_bound >= 1, N * H * W <= CAMO_RGD_MAX_PIXELS: otherwise
 * CAMO_E_ARG. */
int camo_rg_paint(const float* values, int32_t n_nodes, int32_t C, const int32_t* segments, const int32_t* region_map,
                  const int32_t* node_off, int32_t N, int32_t H, int32_t W, int32_t label_bound, float fill, float* maps, void* stream);

/* A predicted map against a ground-truth mask, per image, in TWO launches (a clear and a count, both grids over the whole batch).
 * pred: image i's [H, W] plane starts at pred + i * pred_image_stride floats (H * W for a dense [N, H, W]; one channel of a
 * [N, C, H, W] map is passed in place with stride C * H * W); gt [N, H, W] uint8.  Predicted positive: pred > threshold;
 * ground-truth positive: gt > 127.  counts [N, 5] int64 = TP, FP, FN, TN, A with
 *   A = sum over the pixels of llrint(|pred - g| * 2^32), |pred - g| in double, g in {0, 1}:
 * the absolute-error sum as an integer (pred in [0, 1] and H * W <= 2^26 keep it below 2^58; a pred that is not finite leaves A
 * undefined and is counted as not positive when it is NaN).  Block-level sums, then 64-bit
 * INTEGER atomics: no floating-point atomic is on the path, so the five numbers are functions of the inputs alone (two calls
 * give the same bytes, a batch gives the rows of its images one by one).
 * The ratios are not part of the ABI; the Python surface computes them from the counts in float64 with these conventions:
 *   IoU = TP / (TP + FP + FN), Dice = 2 TP / (2 TP + FP + FN): 1 when the denominator is 0 (both masks empty);
 *   precision = TP / (TP + FP), recall = TP / (TP + FN), F1 = 2 P R / (P + R): 0 when the denominator is 0;
 *   accuracy = (TP + TN) / (H W), MAE = A / 2^32 / (H W).
 * Needs N, H, W >= 1, N <= CAMO_RGD_MAX_IMAGES, H * W <= CAMO_RGD_MAX_IMAGE_PIXELS, pred_image_stride >= H * W, a threshold that is not NaN: otherwise
 * CAMO_E_ARG.  What counts holds on entry is unspecified; every element of it is written. */
int camo_seg_counts(const float* pred, int64_t pred_image_stride, const uint8_t* gt, float threshold, int32_t N, int32_t H, int32_t W,
                    int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
