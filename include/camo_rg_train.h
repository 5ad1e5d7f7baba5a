/* C ABI of the region-graph GNN's loss and gradients on MI355X with the batch-norm statistics frozen, exported by the
 * same libcamo_fusion.so as include/camo_fusion.h (error text: camo_last_error()).
 *
 * The first slice of training the reference's RegionGraphGNN (models/region_graph/train.py): the loss on the three node heads and
 * the whole backward of the network, with every BatchNorm1d using its running statistics and every dropout layer the identity --
 * model.eval() arithmetic plus gradients, i.e. fine-tuning with frozen statistics.  Batch-statistics batch norm and dropout are NOT
 * here (camo_rg_train_bn.h, camo_rg_train_drop.h).  The node targets come from ground-truth masks through the entry point of camo_rg_targets.h; the optimizer step is
 * camo_grad_sumsq + camo_clip_adamw of camo_fusion.h on one flat buffer of these gradients, and any other optimizer
 * can step on the gradient buffers this call writes.
 * PARITY UNPINNED: the reference tree and torch_geometric are absent here, train.py (its loss weights, its targets) cannot be read
 * and no region-graph checkpoint ships.  The text below is the definition; it is restated in torch float64 on the fp32 inputs in
 * tests/rg_train_ref.py, whose autograd gradients the kernels are tested against.
 *
 * Device pointers only, fp32 (targets int32 / fp32), enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok /
 * negative CAMO_E_* as in camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of
 * camo_fusion.h. */
#ifndef CAMO_RG_TRAIN_H
#define CAMO_RG_TRAIN_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_detect.h"
#ifdef __cplusplus
extern "C" {
#endif

/* gradient table: device pointers in this order, each buffer of its parameter's shape.  Slots 0 .. 19: the parameter table of
 * camo_rg_gnn.h without its 8 running-statistic slots; slots 20 .. 31: the head table of camo_rg_detect.h (slot 20 + CAMO_RGD_*). */
enum {
  CAMO_RGT_C1_ATT_SRC = 0, /* conv1.att_src */
  CAMO_RGT_C1_ATT_DST,     /* conv1.att_dst */
  CAMO_RGT_C1_BIAS,        /* conv1.bias */
  CAMO_RGT_C1_W,           /* conv1.lin.weight */
  CAMO_RGT_BN1_W,          /* bn1.weight */
  CAMO_RGT_BN1_B,          /* bn1.bias */
  CAMO_RGT_C2_BIAS,        /* conv2.bias, conv2.lin.weight, bn2.weight, bn2.bias : 4 slots; conv3, conv4 follow */
  CAMO_RGT_FC_W = CAMO_RGT_C2_BIAS + 12, /* fc_shared.weight */
  CAMO_RGT_FC_B,                         /* fc_shared.bias */
  CAMO_RGT_HEADS,                        /* 20: the 12 head gradients, CAMO_RGD_* order */
  CAMO_RGT_NGRADS = CAMO_RGT_HEADS + CAMO_RGD_NPARAMS /* 32 */
};

/* Bytes of workspace camo_rg_loss_backward needs for a graph of N nodes and E CSR entries (self-loops included); 0 when the
 * arguments are out of range (see below). */
size_t camo_rg_train_workspace_bytes(const camo_rg_dims_t* dims, int32_t num_classes, int32_t N, int32_t E);

/* Forward, loss and backward in one call.
 *
 * Forward: exactly what camo_rg_node_embeddings followed by camo_rg_node_heads computes (camo_rg_gnn.h, camo_rg_detect.h), except
 * that the softmax of the attention uses expf on the row maximum taken first (not the online form with the fast exponential) and
 * that the second layer of each head adds its products in a fixed order of its own.  `params` is the 28-slot table of camo_rg_gnn.h
 * (running_mean and running_var are read and never written), `head_params` the 12-slot table of camo_rg_detect.h.
 *
 * Loss: per node v the targets are mask_t[v] and inst_t[v], int32 in [0, num_classes) or -1 for an ignored node (any value
 * outside [0, num_classes) is ignored), and edge_t[v], fp32 in [0, 1] or negative for an ignored node.
 *   L = w_m CE(l_mask, mask_t) + w_i CE(l_instance, inst_t) + w_e BCEWithLogits(l_edge, edge_t),
 * each term the mean over its non-ignored nodes; a term whose nodes are all ignored is 0 and has zero gradient.
 *   CE(l, t) = max(l) + logf(sum_c expf(l_c - max(l))) - l_t      BCE(z, t) = max(z, 0) - z t + logf(1 + expf(-|z|))
 * The non-ignored counts are integers; the sums over the nodes are taken in double in a fixed order.
 * loss[4] = total, mask term, instance term, edge term (the terms unweighted).
 *
 * Gradients: grads[CAMO_RGT_NGRADS] buffers, each OVERWRITTEN with dL/dparameter (BatchNorm weight and bias included; no gradient
 * is taken for x or for the edge weights).  ReLU passes a gradient where its output is > 0, the attention's leaky ReLU has slope 1
 * where its argument is > 0 and 0.2 elsewhere.  Exact fp32: products and sums in fp32 (the dense products through the exact-fp32
 * matrix kernels), every sum over nodes or edges owned by one thread or wave and added in a fixed order -- no floating-point
 * atomic is on the path, so losses and gradients are functions of the input arrays alone (two calls give the same bytes).
 *
 * Graph: rowptr / col / w is the CSR by TARGET that camo_rg_gnn.h's builder gives, one self-loop per node, E entries; rrowptr / rcol / rw is the
 * CSR of the REVERSED graph -- row j lists the targets i of the edges j -> i -- which the same builder gives when the two rows of
 * edge_index are swapped.  The two MUST describe the same edge multiset (same pairs, same weights, same E); this is not checked.
 * Several graphs batch as one block-diagonal graph; the means then run over all its nodes.
 *
 * Needs N >= 1, E >= N, in_channels >= 1, 2 <= hidden <= 512 and even, 1 <= heads <= 8, 2 <= num_classes <= 8
 * (CAMO_E_UNSUPPORTED otherwise), non-null pointers and finite loss weights (CAMO_E_ARG), and workspace_bytes >=
 * camo_rg_train_workspace_bytes() (CAMO_E_WORKSPACE). */
int camo_rg_loss_backward(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                          const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                          const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                          const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                          float* loss, float* const* grads, void* stream);

#ifdef __cplusplus
}
#endif
#endif
