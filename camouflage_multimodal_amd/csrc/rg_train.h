// Kernels of the region-graph GNN's loss and backward (rg_train.hip) with frozen batch-norm statistics (include/camo_rg_train.h,
// DESIGN.md 9a) or with batch statistics (include/camo_rg_train_bn.h): the saving variant of the GAT aggregation, the loss on the node heads, the backward of the aggregations
// over the reversed CSR, and the fixed-order column sums behind every bias / batch-norm / attention-vector gradient.  No
// floating-point atomic anywhere: every sum has one owner and a fixed order.  All launchers return hipError_t as int; the callers
// have checked the arguments.
#pragma once
#include "rg_gnn.h"

// Dropout of the training forward (include/camo_rg_train_drop.h): one DropCfg per class, all of one seed; a class with p == 0 is off
// and runs the kernels without dropout.  The backward needs the three scales only (the saved activations are the dropped ones).
struct RgDropout { DropCfg conv, shared, head; };

constexpr int RGT_ROWS = 64;        // node rows per block of the first stage of a column sum
inline int rgt_row_blocks(int N) { return (N + RGT_ROWS - 1) / RGT_ROWS; }

// GAT aggregate that keeps what the backward needs: m, S [N, heads] softmax maximum and denominator per target and head,
// O [N, heads, C] per-head aggregates, xhat [N, C] = (pre - mean) / sqrt(var + 1e-5), out [N, C] = relu(xhat * weight + bias_bn).
// raw: xhat = pre and nothing else -- bn is not read and out is not written (batch statistics; m, S, O are saved all the same)
// drop (not raw; include/camo_rg_train_drop.h): out[i, c] *= drop_mult(*drop, site, i * C + c) after the ReLU, xhat undropped
int launch_rgt_gat_forward(const float* Hh, const float* a_src, const float* a_dst, const int* rowptr, const int* col, const float* bias,
                           BnEval bn, float* m, float* S, float* O, float* xhat, float* out, int N, int heads, int C, hipStream_t stream,
                           bool raw = false, const DropCfg* drop = nullptr, uint32_t site = 0);
// (the GCN aggregate that keeps xhat is rg_gnn.h's launch_gcn_aggregate with a non-null xhat)
// copies the three heads' first layers into one [3 hidden / 2, hidden] weight and one [3 hidden / 2] bias
int launch_rgt_concat_heads(const float* const* hp, float* W1, float* b1, int hidden, hipStream_t stream);
// logits [N, 2 nc + 1] from Z [N, 3 hidden / 2] (the heads' hidden activations): one wave per node
int launch_rgt_head_logits(const float* const* hp, const float* Z, float* logits, int N, int hidden, int nc, hipStream_t stream);
// ONE block: the non-ignored counts (integers), the three means and the total -> loss[4]; dlogits [N, 2 nc + 1] already scaled by
// weight / count
int launch_rgt_loss(const float* logits, const int* mask_t, const int* inst_t, const float* edge_t, float wm, float wi, float we, int N,
                    int nc, float* loss, float* dlogits, hipStream_t stream);
// The structure loss on the painted mask (include/camo_rg_pixel_loss.h): node_w [N, 2] int64 = (A, B) per node, node_off
// [n_images + 1] (clamped to [0, N] on the device).  TWO launches after launch_rgt_loss, nc == 2: one block per image adds
// w_pixel dP/dz to dlogits[v][1] and subtracts it from dlogits[v][0]; one block adds w_pixel P to loss[0] and writes loss[4], loss[5]
// = mean wbce, mean wiou.  w_pixel == 0: dlogits and loss[0] keep their bytes.
struct RgPixel { const long long* node_w; const int* node_off; int n_images; int radius; float w_pixel; };
int launch_rgt_pixel_loss(const float* logits, const RgPixel& px, int N, int nc, float* loss, float* dlogits, hipStream_t stream);
// dZ [N, 3 hidden / 2] = (Z > 0 ? scale : 0) * dlogits_h . W2_h   (scale: 1, or 1 / (1 - p_head) when Z is the dropped activation)
int launch_rgt_head_dz(const float* const* hp, const float* Z, const float* dlogits, float* dZ, int N, int hidden, int nc, hipStream_t stream,
                       float scale = 1.f);

// partial[b, m * NB + c] = sum over the rows r of block b of A[r * lda + m] * B[r * ldb + c]   (A null: ones, MA = 1)
int launch_rgt_cross_partial(const float* A, int lda, int MA, const float* B, int ldb, int NB, int N, float* partial, hipStream_t stream);
// out[c] = sum_b partial[b, c] in increasing b, c < width, written to up to 4 segments: segment s takes columns [beg[s], beg[s + 1])
struct RgtSegs { float* out[4]; int beg[5]; int n; };
int launch_rgt_colsum_finish(const float* partial, int nb, int width, RgtSegs segs, hipStream_t stream);

// in place d = d * weight / sqrt(var + 1e-5) (d arrives ReLU-masked: it is dy); partial[b, 0 | 1, c] = sum dy * xhat | sum dy.
// batch: the partial sums only -- d stays dy and bn is not read
int launch_rgt_bn_backward(float* d, const float* xhat, BnEval bn, int N, int C, float* partial, hipStream_t stream, bool batch = false);
// dweight = sum0, dbias_bn = sum1, dbias_conv = sum1 * weight / sqrt(var + 1e-5); batch: dbias_conv = +0.0f and bn is not read
int launch_rgt_bn_finish(const float* partial, int nb, BnEval bn, int C, float* dweight, float* dbias_bn, float* dbias_conv, hipStream_t stream,
                         bool batch = false);

// Batch statistics of z [N, C], N >= 2, in two launches: per block of RGT_ROWS rows (mean, sum of centred squares) in row order ->
// partial [row blocks, 2, C]; then per channel 16 contiguous runs of blocks are merged in block order (Chan) and the 16 runs in run
// order, by one owner, which writes mean[c],
// rstd[c] = 1 / sqrt(var + 1e-5) (var = M2 / N), batch_stats[0 | 1, c] = mean | var if non-null, and, if running_mean is non-null,
// running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with var N / (N - 1)
int launch_rgt_bn_stats(const float* z, int N, int C, float momentum, float* partial, float* mean, float* rstd, float* batch_stats,
                        float* running_mean, float* running_var, hipStream_t stream);
// in place zx = xhat = (z - mean) rstd; out = relu(xhat weight + bias), times drop_mult(*drop, site, r * C + c) when drop is given
int launch_rgt_bn_apply(float* zx, const float* mean, const float* rstd, const float* weight, const float* bias, float* out, int N, int C,
                        hipStream_t stream, const DropCfg* drop = nullptr, uint32_t site = 0);
// in place d = weight rstd (d - dbias / N - xhat dweight / N): dy -> dz once dweight = sum dy xhat and dbias = sum dy are finished
int launch_rgt_bn_dz(float* d, const float* xhat, const float* weight, const float* rstd, const float* dweight, const float* dbias, int N, int C,
                     hipStream_t stream);

// dXW[j, :] = sum over the edges j -> i of the REVERSED CSR (row j: targets i, weights w) dinv[j] w dinv[i] dPre[i, :]
int launch_rgt_gcn_backward(const float* dPre, const int* rrowptr, const int* rcol, const float* rw, const float* dinv, float* dXW, int N,
                            int C, hipStream_t stream);
// pass A over the CSR by target: r[i, k] = <g[i], O[i, k, :]>, da_dst[i, k] = sum_j ds   (g = dPre / heads)
int launch_rgt_gat_backward_a(const float* dPre, const float* Hh, const float* O, const float* a_src, const float* a_dst, const float* m,
                              const float* S, const int* rowptr, const int* col, float* r, float* da_dst, int N, int heads, int C,
                              hipStream_t stream);
// pass B over the reversed CSR: da_src[j, k] = sum_i ds, dh[j, k, :] = sum_i alpha g[i] + da_src att_src[k] + da_dst att_dst[k]
int launch_rgt_gat_backward_b(const float* dPre, const float* Hh, const float* a_src, const float* a_dst, const float* m, const float* S,
                              const float* r, const float* da_dst, const float* att_src, const float* att_dst, const int* rrowptr,
                              const int* rcol, float* da_src, float* dh, int N, int heads, int C, hipStream_t stream);
// partial[b, 0 | 1, k, c] = sum over the rows n of block b of da_src[n, k] Hh[n, k, c] | da_dst[n, k] Hh[n, k, c]
int launch_rgt_att_partial(const float* da_src, const float* da_dst, const float* Hh, int N, int heads, int C, float* partial,
                           hipStream_t stream);
