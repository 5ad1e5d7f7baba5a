/* C ABI of the region-graph GNN's loss and gradients on MI355X with BATCH-STATISTICS batch norm, exported by the same
 * libcamo_fusion.so as include/camo_fusion.h (error text: camo_last_error()).
 *
 * The second slice of training the reference's RegionGraphGNN (models/region_graph/train.py, which trains under model.train()):
 * camo_rg_train.h's call with every BatchNorm1d normalising by the statistics of the call's own nodes and updating its running
 * statistics, so that training from fresh weights produces the statistics the inference path (camo_rg_node_embeddings) reads.
 * Dropout is NOT here: every dropout layer is the identity, as in camo_rg_train.h (camo_rg_train_drop.h is this call with dropout).
 * PARITY UNPINNED: the reference tree and torch_geometric are absent here, train.py cannot be read and no region-graph checkpoint
 * ships.  The text below is the definition; it is restated in torch float64 on the fp32 inputs in tests/rg_train_bn_ref.py, whose
 * batch-norm step is held to torch.nn.functional.batch_norm(training=True) and whose autograd gradients the kernels are tested
 * against.
 *
 * Device pointers only, fp32 (targets int32 / fp32), enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok /
 * negative CAMO_E_* as in camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of
 * camo_fusion.h. */
#ifndef CAMO_RG_TRAIN_BN_H
#define CAMO_RG_TRAIN_BN_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_train.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace camo_rg_loss_backward_bn needs: camo_rg_train_workspace_bytes plus 4 * 2 * hidden floats (mean and
 * 1 / sqrt(var + 1e-5) of the four layers); 0 when the arguments are out of range (see below). */
size_t camo_rg_train_bn_workspace_bytes(const camo_rg_dims_t* dims, int32_t num_classes, int32_t N, int32_t E);

/* Forward, loss and backward in one call, batch norm on batch statistics.
 *
 * Everything is camo_rg_loss_backward's (camo_rg_train.h) -- the GAT and GCN aggregations, fc_shared, the heads, the loss with its
 * ignore rules and integer counts, loss[4], the 32-entry gradient table, the two CSRs -- except the four batch norms.  For each of
 * them let z [N, C] be the conv output INCLUDING its bias, N all the nodes of the call (a block-diagonal batch is one population,
 * as BatchNorm1d on a batch of graphs is):
 *   mu_c   = (1 / N) sum_n z[n, c]
 *   var_c  = (1 / N) sum_n (z[n, c] - mu_c)^2                       (biased)
 *   xhat   = (z - mu) / sqrt(var + 1e-5)
 *   out    = relu(weight xhat + bias)
 * and backward, dy being the gradient of `weight xhat + bias` (the ReLU-masked gradient of out):
 *   dweight = sum_n dy xhat      dbias = sum_n dy
 *   dz      = weight / sqrt(var + 1e-5) (dy - dbias / N - xhat dweight / N)
 * The variance is never taken as E[z^2] - mu^2: per block of 64 rows the mean and the sum of centred squares in row order, the
 * blocks merged in block order (Chan's update), in fp32.
 *
 * The four conv biases (conv1.bias .. conv4.bias) cancel against the mean: the loss does not depend on them.  Their four gradient
 * buffers (CAMO_RGT_C1_BIAS, CAMO_RGT_C2_BIAS and the two that follow at + 4 and + 8) are written as exact +0.0f, not as the
 * rounding noise a sum over dz would leave.
 *
 * `params`: the 28-slot table of camo_rg_gnn.h; its 8 running-statistic slots are NOT read (they may be null).
 * `running`: 8 device pointers, bn1 mean, bn1 var, bn2 mean, ... bn4 var, each [hidden], updated in place
 *   running_mean <- (1 - momentum) running_mean + momentum mu
 *   running_var  <- (1 - momentum) running_var  + momentum var N / (N - 1)
 * by the thread that finishes the channel's statistics; null: no update (momentum is then not looked at).
 * `batch_stats`: [4][2][hidden] receives mu, then the biased var, of each layer; null: not written.
 *
 * As in camo_rg_train.h no floating-point atomic is on the path: every output element has one owner and a fixed order, so losses,
 * gradients, batch_stats and the updated running statistics are functions of the input arrays alone (two calls on the same CSR
 * arrays give the same bytes).
 *
 * Needs N >= 2, E >= N, in_channels >= 1, 2 <= hidden <= 512 and even, 1 <= heads <= 8, 2 <= num_classes <= 8
 * (CAMO_E_UNSUPPORTED otherwise), non-null pointers (running and batch_stats excepted; with running given, all 8 of its entries),
 * finite loss weights, momentum finite and in (0, 1] when running is given (CAMO_E_ARG), and workspace_bytes >=
 * camo_rg_train_bn_workspace_bytes() (CAMO_E_WORKSPACE). */
int camo_rg_loss_backward_bn(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                             const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                             const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                             const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                             float* loss, float* const* grads, float momentum, float* const* running, float* batch_stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
