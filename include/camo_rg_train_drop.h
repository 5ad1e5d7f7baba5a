/* C ABI of the region-graph GNN's loss and gradients on MI355X WITH DROPOUT, exported by the same libcamo_fusion.so
 * as include/camo_fusion.h (error text: camo_last_error()).
 *
 * The last slice of training the reference's RegionGraphGNN under model.train() (models/region_graph/train.py): the call of
 * camo_rg_train.h (batch norm frozen) or of camo_rg_train_bn.h (batch statistics) with inverted dropout after every ReLU that the
 * model's heads and trunk carry a dropout layer behind.
 * PARITY UNPINNED: the reference tree and torch_geometric are absent here, train.py (its dropout rates) cannot be read and no
 * region-graph checkpoint ships, so the rates are the caller's to state, in three classes.  The text below is the definition; it is
 * restated in torch float64 on the fp32 inputs in tests/rg_train_drop_ref.py, whose autograd gradients the kernels are tested
 * against.
 *
 * Device pointers only, fp32 (targets int32 / fp32), enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok /
 * negative CAMO_E_* as in camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of
 * camo_fusion.h. */
#ifndef CAMO_RG_TRAIN_DROP_H
#define CAMO_RG_TRAIN_DROP_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_train_bn.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Dropout sites: one independent mask stream each.  (The fusion model's sites are 1 .. 11, camo_fusion.h's dropout definition.)
 *
 *   class     site                              tensor and element index
 *   p_conv    CAMO_RGT_SITE_CONV0 + k, k = 0..3  h[k] [N, hidden], the output of conv(k + 1) -> bn -> relu:   n * hidden + c
 *   p_shared  CAMO_RGT_SITE_SHARED               emb [N, hidden] = relu(fc_shared(h[3])):                    n * hidden + c
 *   p_head    CAMO_RGT_SITE_HEADS                Z [N, 3 hidden / 2] = relu of the three heads' first layers,
 *                                                concatenated mask | instance | edge:                        n * (3 hidden / 2) + u */
#define CAMO_RGT_SITE_CONV0 32
#define CAMO_RGT_SITE_SHARED 36
#define CAMO_RGT_SITE_HEADS 37

/* Bytes of workspace camo_rg_loss_backward_drop needs: camo_rg_train_workspace_bytes (batch_stats == 0) or
 * camo_rg_train_bn_workspace_bytes (batch_stats != 0) -- nothing more is saved; 0 when the arguments are out of range. */
size_t camo_rg_train_drop_workspace_bytes(const camo_rg_dims_t* dims, int32_t num_classes, int32_t N, int32_t E, int32_t batch_stats);

/* Forward, loss and backward in one call, with dropout.
 *
 * batch_stats_mode 0: everything is camo_rg_loss_backward's (camo_rg_train.h); momentum is not looked at and `running` and
 * `batch_stats` must be null.  batch_stats_mode 1: everything is camo_rg_loss_backward_bn's (camo_rg_train_bn.h), `momentum`,
 * `running` and `batch_stats` included.  Any other mode: CAMO_E_ARG.  On top of either, at each of the eight sites above, with p the
 * rate of the site's class and y the ReLU's output,
 *   y_d[idx] = y[idx] * (keep(site, idx) ? 1.0f / (1.0f - p) : 0)          (the multiplier rounded to fp32 once)
 *   keep(site, idx) = fmix32((idx + site * 0x85EBCA77 + seed_lo) ^ seed_hi) >= thr,   thr = ceil(p * 2^24) << 8
 * in 32-bit unsigned arithmetic, fmix32 the murmur3 finaliser (x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35;
 * x ^= x >> 16) and seed_lo / seed_hi the halves of `seed`: the mask definition of camo_fusion.h's dropout, i.e. keep iff the top 24
 * bits of the hash, as a fraction of 2^24, are >= p.  The layers after a site read y_d.  Batch statistics are taken before their
 * layer's dropout (of the conv output, as in camo_rg_train_bn.h), so they see the dropout of the layers below only.
 * Backward: the gradient of y is the gradient of y_d times the same multiplier; as y_d > 0 exactly where the element was kept and
 * the ReLU is open, the saved y_d is the only mask there is -- no mask is stored or drawn a second time.  A class whose rate is 0
 * has no dropout and runs the kernels of the call without it.
 *
 * With all three rates 0 the call IS the mode's existing entry: the same launches of the same kernels, the same bytes.
 * As there, no floating-point atomic is on the path: two calls on the same arrays with the same seed give the same bytes.
 *
 * Needs what the mode's entry needs, each rate finite and in [0, 1) (CAMO_E_ARG), N * (3 hidden / 2) < 2^32 (the element indices are
 * 32-bit: CAMO_E_UNSUPPORTED), and workspace_bytes >= camo_rg_train_drop_workspace_bytes() (CAMO_E_WORKSPACE). */
int camo_rg_loss_backward_drop(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                               const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                               const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                               const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                               float* loss, float* const* grads, float momentum, float* const* running, float* batch_stats,
                               int32_t batch_stats_mode, float p_conv, float p_shared, float p_head, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif
