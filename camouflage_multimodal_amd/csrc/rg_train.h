// Kernels of the region-graph GNN's loss and backward with frozen batch-norm statistics (rg_train.hip, include/camo_rg_train.h,
// DESIGN.md 9a): the saving variant of the GAT aggregation, the loss on the node heads, the backward of the aggregations
// over the reversed CSR, and the fixed-order column sums behind every bias / batch-norm / attention-vector gradient.  No
// floating-point atomic anywhere: every sum has one owner and a fixed order.  All launchers return hipError_t as int; the callers
// have checked the arguments.
#pragma once
#include "rg_gnn.h"

constexpr int RGT_ROWS = 64;        // node rows per block of the first stage of a column sum
inline int rgt_row_blocks(int N) { return (N + RGT_ROWS - 1) / RGT_ROWS; }

// GAT aggregate that keeps what the backward needs: m, S [N, heads] softmax maximum and denominator per target and head,
// O [N, heads, C] per-head aggregates, xhat [N, C] = (pre - mean) / sqrt(var + 1e-5), out [N, C] = relu(xhat * weight + bias_bn)
int launch_rgt_gat_forward(const float* Hh, const float* a_src, const float* a_dst, const int* rowptr, const int* col, const float* bias,
                           BnEval bn, float* m, float* S, float* O, float* xhat, float* out, int N, int heads, int C, hipStream_t stream);
// (the GCN aggregate that keeps xhat is rg_gnn.h's launch_gcn_aggregate with a non-null xhat)
// copies the three heads' first layers into one [3 hidden / 2, hidden] weight and one [3 hidden / 2] bias
int launch_rgt_concat_heads(const float* const* hp, float* W1, float* b1, int hidden, hipStream_t stream);
// logits [N, 2 nc + 1] from Z [N, 3 hidden / 2] (the heads' hidden activations): one wave per node
int launch_rgt_head_logits(const float* const* hp, const float* Z, float* logits, int N, int hidden, int nc, hipStream_t stream);
// ONE block: the non-ignored counts (integers), the three means and the total -> loss[4]; dlogits [N, 2 nc + 1] already scaled by
// weight / count
int launch_rgt_loss(const float* logits, const int* mask_t, const int* inst_t, const float* edge_t, float wm, float wi, float we, int N,
                    int nc, float* loss, float* dlogits, hipStream_t stream);
// dZ [N, 3 hidden / 2] = (Z > 0) * dlogits_h . W2_h
int launch_rgt_head_dz(const float* const* hp, const float* Z, const float* dlogits, float* dZ, int N, int hidden, int nc, hipStream_t stream);

// partial[b, m * NB + c] = sum over the rows r of block b of A[r * lda + m] * B[r * ldb + c]   (A null: ones, MA = 1)
int launch_rgt_cross_partial(const float* A, int lda, int MA, const float* B, int ldb, int NB, int N, float* partial, hipStream_t stream);
// out[c] = sum_b partial[b, c] in increasing b, c < width, written to up to 4 segments: segment s takes columns [beg[s], beg[s + 1])
struct RgtSegs { float* out[4]; int beg[5]; int n; };
int launch_rgt_colsum_finish(const float* partial, int nb, int width, RgtSegs segs, hipStream_t stream);

// in place d = d * weight / sqrt(var + 1e-5) (d arrives ReLU-masked: it is dy); partial[b, 0 | 1, c] = sum dy * xhat | sum dy
int launch_rgt_bn_backward(float* d, const float* xhat, BnEval bn, int N, int C, float* partial, hipStream_t stream);
// dweight = sum0, dbias_bn = sum1, dbias_conv = sum1 * weight / sqrt(var + 1e-5)
int launch_rgt_bn_finish(const float* partial, int nb, BnEval bn, int C, float* dweight, float* dbias_bn, float* dbias_conv, hipStream_t stream);

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
