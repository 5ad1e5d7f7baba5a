// C ABI of the region-graph side (include/camo_rg_*.h, camo_canny.h, camo_slic.h): argument checks, workspace carving and the launch
// sequences of the CSR build, the GNN embedding path, region-graph construction, Canny, SLIC, the node heads / painting / metrics, the
// GNN's training call (four entries, one sequence: rgt_run) and the node targets and weights from ground-truth masks.  The image
// pipeline around the detector has image_abi.hip.  No device code here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "abi_util.h"
#include "rg_gnn.h"
#include "rg_features.h"
#include "rg_batch.h"
#include "canny.h"
#include "slic.h"
#include "rg_detect.h"
#include "rg_train.h"
#include "rg_targets.h"
#include "rg_pixel_loss.h"
#include "../../include/camo_rg_gnn.h"
#include "../../include/camo_rg_features.h"
#include "../../include/camo_rg_batch.h"
#include "../../include/camo_canny.h"
#include "../../include/camo_slic.h"
#include "../../include/camo_rg_detect.h"
#include "../../include/camo_rg_train.h"
#include "../../include/camo_rg_train_bn.h"
#include "../../include/camo_rg_train_drop.h"
#include "../../include/camo_rg_targets.h"
#include "../../include/camo_rg_pixel_loss.h"

using namespace camo_abi;

// ---- Region-Graph GNN embedding path (include/camo_rg_gnn.h) ----------------------------------------------
namespace {
// The embedding forward's buffers: h[k] = output of conv(k + 1) after batch norm and ReLU.  xhat (the normalised pre-activations) and the
// GAT saves m, S, O are the training call's; all null at inference.
struct RgFwd { float *Hh, *a_src, *a_dst, *dinv, *xw, *h[4], *xhat[4], *m, *S, *O; };

// Batch-statistics mode of the forward (include/camo_rg_train_bn.h): stats [4][2][C] receives mean | rstd of every layer for the
// backward, partial is the column sums' first-stage buffer; running (8 pointers, or null) is updated in place, batch_stats
// ([4][2][C] mean | biased var, or null) is the caller's.
struct RgBatchNorm { float* stats; float* partial; float* const* running; float momentum; float* batch_stats; };

struct RgWs : RgFwd { size_t bytes; };
RgWs rg_carve(const camo_rg_dims_t& d, int N, void* base) {
  RgWs w{};
  Carver c(base);
  const size_t n = N, C = d.hidden, K = d.heads;
  w.Hh = c.take<float>(n * K * C); w.a_src = c.take<float>(n * K); w.a_dst = c.take<float>(n * K); w.dinv = c.take<float>(n);
  w.xw = c.take<float>(n * C);
  w.h[0] = w.h[2] = c.take<float>(n * C); w.h[1] = w.h[3] = c.take<float>(n * C);      // ping-pong: a layer reads one and writes the other
  w.bytes = c.bytes();
  return w;
}
int rg_check(const camo_rg_dims_t* d, int N) {
  if (!d) return fail(CAMO_E_ARG, "dims is null");
  if (N < 1 || d->in_channels < 1 || d->hidden < 1 || d->hidden > 512 || d->heads < 1 || d->heads > 8)
    return fail(CAMO_E_UNSUPPORTED, "need N >= 1, hidden <= 512, 1 <= heads <= 8");
  return 0;
}

// x -> h[3] (conv1 .. conv4, each with its batch norm and ReLU), then fc_shared + ReLU -> emb.  bb null: batch norm on the running
// statistics, inside the aggregation kernels.  bb given (needs the saving buffers of f): the aggregations write the raw
// pre-activation z to xhat[k], then the statistics of z over the N rows, then xhat in place and h[k] = relu(xhat weight + bias).
// dr given (needs the saving buffers of f; include/camo_rg_train_drop.h): h[k] and emb leave their ReLU through inverted dropout, in the
// kernel that applies the ReLU -- the saving aggregations (frozen), bn_apply (batch statistics), the fc_shared GEMM's epilogue.  A
// class with p == 0 runs the kernels without dropout.
int rg_forward(const camo_rg_dims_t& d, const float* const* P, const float* x, const int32_t* rowptr, const int32_t* col, const float* w,
               int N, const RgFwd& f, float* emb, hipStream_t st, const RgBatchNorm* bb = nullptr, const RgDropout* dr = nullptr) {
  const int C = d.hidden, K = d.heads, In = d.in_channels;
  const bool raw = bb != nullptr;
  if (dr && !f.m) return fail(CAMO_E_ARG, "dropout needs the saving forward");
  const DropCfg* dconv = dr && dr->conv.p > 0.f ? &dr->conv : nullptr;
  const bool dshared = dr && dr->shared.p > 0.f;
  auto bn = [&](int slot) { return BnEval{P[slot], P[slot + 1], P[slot + 2], P[slot + 3]}; };
  auto batch_norm = [&](int layer, int slot) -> int {      // slot: the layer's batch-norm weight
    if (!raw) return 0;
    float* mean = bb->stats + (size_t)layer * 2 * C;
    CK(launch_rgt_bn_stats(f.xhat[layer], N, C, bb->momentum, bb->partial, mean, mean + C,
                           bb->batch_stats ? bb->batch_stats + (size_t)layer * 2 * C : nullptr, bb->running ? bb->running[2 * layer] : nullptr,
                           bb->running ? bb->running[2 * layer + 1] : nullptr, st), "batch statistics");
    CK(launch_rgt_bn_apply(f.xhat[layer], mean, mean + C, P[slot], P[slot + 1], f.h[layer], N, C, st, dconv, SITE_RGT_CONV0 + layer), "batch norm");
    return 0;
  };
  GB g(dshared ? dr->shared : make_drop(0, 0.f, 0), CAMO_PREC_F32, st);
  // conv1: GATConv (extract_rg_embeddings.py:104) + bn1 + relu
  g.nt(x, In, P[CAMO_RG_C1_W], In, nullptr, f.Hh, K * C, N, K * C, In);
  CK(g.run(), "gat projection");
  CK(launch_gat_alpha(f.Hh, P[CAMO_RG_C1_ATT_SRC], P[CAMO_RG_C1_ATT_DST], f.a_src, f.a_dst, N, K, C, st), "gat attention logits");
  // Two GAT kernels on purpose: inference runs an online softmax with __expf, training a two-pass softmax with expf because its
  // backward recomputes alpha from the saved m and S.  One kernel for both would change one path's bits.
  const float* b1 = P[CAMO_RG_C1_BIAS];
  CK(f.m ? launch_rgt_gat_forward(f.Hh, f.a_src, f.a_dst, rowptr, col, b1, bn(CAMO_RG_BN1), f.m, f.S, f.O, f.xhat[0], f.h[0], N, K, C, st, raw,
                                  raw ? nullptr : dconv, SITE_RGT_CONV0)
         : launch_gat_aggregate(f.Hh, f.a_src, f.a_dst, rowptr, col, b1, bn(CAMO_RG_BN1), f.h[0], N, K, C, st), "gat aggregate");
  if (int e = batch_norm(0, CAMO_RG_BN1)) return e;
  // conv2..4: GCNConv with edge weights (:108-118) + bn + relu
  CK(launch_gcn_dinv(rowptr, w, f.dinv, N, st), "gcn degrees");
  for (int k = 0; k < 3; ++k) {
    const int base = CAMO_RG_C2_BIAS + 6 * k;
    g.nt(f.h[k], C, P[base + 1], C, nullptr, f.xw, C, N, C, C);
    CK(g.run(), "gcn projection");
    CK(launch_gcn_aggregate(f.xw, rowptr, col, w, f.dinv, P[base], bn(base + 2), f.xhat[k + 1], f.h[k + 1], N, C, st, raw,
                            raw ? nullptr : dconv, SITE_RGT_CONV0 + k + 1), "gcn aggregate");
    if (int e = batch_norm(k + 1, base + 2)) return e;
  }
  // fc_shared + relu (:121)
  g.nt(f.h[3], C, P[CAMO_RG_FC_W], C, P[CAMO_RG_FC_B], emb, C, N, C, C, dshared ? GF_RELU | GF_DROPOUT : GF_RELU).drop_site = SITE_RGT_SHARED;
  CK(g.run(), "fc_shared");
  return 0;
}

// camo_rg_loss_backward (include/camo_rg_train.h), camo_rg_loss_backward_bn (include/camo_rg_train_bn.h)
struct RgtWs : RgFwd {      // the forward's buffers, all saved, and the backward's; stats [4][2][C] = mean | rstd: batch statistics only
  float *dh, *r, *da_src, *da_dst, *emb, *Z, *dZ, *logits, *dlogits, *dA, *dB, *W1, *b1, *partial, *stats;
  size_t bytes;
};
size_t rgt_partial_width(const camo_rg_dims_t& d, int nc) {
  const size_t C = d.hidden, K = d.heads, Hh = C / 2;
  return std::max(std::max(2 * K * C, 3 * Hh), std::max((size_t)nc * Hh, (size_t)2 * nc + 1));
}
RgtWs rgt_carve(const camo_rg_dims_t& d, int nc, int N, void* base, bool batch_stats = false) {
  RgtWs w{};
  Carver c(base);
  const size_t n = N, C = d.hidden, K = d.heads, units = 3 * (C / 2), L = 2 * (size_t)nc + 1;
  w.Hh = c.take<float>(n * K * C); w.O = c.take<float>(n * K * C); w.dh = c.take<float>(n * K * C);
  w.a_src = c.take<float>(n * K); w.a_dst = c.take<float>(n * K); w.m = c.take<float>(n * K); w.S = c.take<float>(n * K);
  w.r = c.take<float>(n * K); w.da_src = c.take<float>(n * K); w.da_dst = c.take<float>(n * K); w.dinv = c.take<float>(n);
  w.xw = c.take<float>(n * C);
  for (int k = 0; k < 4; ++k) { w.h[k] = c.take<float>(n * C); w.xhat[k] = c.take<float>(n * C); }
  w.emb = c.take<float>(n * C); w.Z = c.take<float>(n * units); w.dZ = c.take<float>(n * units);
  w.logits = c.take<float>(n * L); w.dlogits = c.take<float>(n * L); w.dA = c.take<float>(n * C); w.dB = c.take<float>(n * C);
  w.W1 = c.take<float>(units * C); w.b1 = c.take<float>(units);
  w.partial = c.take<float>((size_t)rgt_row_blocks(N) * rgt_partial_width(d, nc));
  if (batch_stats) w.stats = c.take<float>(4 * 2 * C);
  w.bytes = c.bytes();
  return w;
}
// rg_check's envelope, plus E >= N and an even hidden, hence >= 2; under batch statistics N >= 2 as well: the unbiased variance of the
// running update divides by N - 1.  The message states the whole of it.
int rgt_check(const camo_rg_dims_t* d, int nc, int N, int E, bool batch) {
  if (!d) return fail(CAMO_E_ARG, "dims is null");
  if (rg_check(d, N) || (batch && N < 2) || E < N || (d->hidden & 1))
    return fail(CAMO_E_UNSUPPORTED,
                batch ? "need N >= 2 (batch statistics), E >= N (one self-loop per node), hidden even and in [2, 512], 1 <= heads <= 8"
                      : "need N >= 1, E >= N (one self-loop per node), hidden even and in [2, 512], 1 <= heads <= 8");
  if (nc < 2 || nc > CAMO_RGD_MAX_CLASSES) return fail(CAMO_E_UNSUPPORTED, "num_classes must be in [2, 8]");
  return 0;
}
size_t rgt_workspace_bytes(const camo_rg_dims_t* d, int nc, int N, int E, bool batch) {      // the three camo_rg_train*_workspace_bytes
  if (rgt_check(d, nc, N, E, batch)) return 0;
  return rgt_carve(*d, nc, N, nullptr, batch).bytes;
}
constexpr bool rg_running_slot(int i) {      // the 8 running-statistic slots of camo_rg_gnn.h's table
  return i == CAMO_RG_BN1 + 2 || i == CAMO_RG_BN1 + 3 || (i >= CAMO_RG_C2_BIAS && i < CAMO_RG_FC_W && (i - CAMO_RG_C2_BIAS) % 6 >= 4);
}
static_assert(rg_running_slot(6) && rg_running_slot(7) && rg_running_slot(12) && rg_running_slot(25) && !rg_running_slot(5) && !rg_running_slot(8) &&
              !rg_running_slot(11) && !rg_running_slot(26), "the running statistics are slots 6, 7, then 12, 13 of every six");

// The 24 arguments the four training entries share, in ABI order (include/camo_rg_train.h): every entry fills one.
struct RgtCall {
  const camo_rg_dims_t* dims; int32_t num_classes; const float* const* params; const float* const* head_params;
  const float* x; const int32_t* rowptr; const int32_t* col; const float* w; const int32_t* rrowptr; const int32_t* rcol; const float* rw;
  int32_t N, E; const int32_t* mask_t; const int32_t* inst_t; const float* edge_t; float w_mask, w_instance, w_edge;
  void* workspace; size_t workspace_bytes; float* loss; float* const* grads; void* stream;
};

// What camo_rg_node_targets and camo_rg_pixel_weights share: the sizes of the label maps, and (after each entry's own scalars) the maps.
int rg_maps_sizes(int N, int H, int W, int label_bound, int n_nodes) {
  if (N < 1) return fail(CAMO_E_ARG, "N must be >= 1");
  if (H < 1) return fail(CAMO_E_ARG, "H must be >= 1");
  if (W < 1) return fail(CAMO_E_ARG, "W must be >= 1");
  if (label_bound < 1 || label_bound > CAMO_RG_MAX_LABELS) return fail(CAMO_E_ARG, "label_bound must be in [1, CAMO_RG_MAX_LABELS]");
  if (n_nodes < 1) return fail(CAMO_E_ARG, "n_nodes must be >= 1");
  if ((long long)H * W > CAMO_RGB_MAX_IMAGE_PIXELS) return fail(CAMO_E_ARG, "H * W exceeds CAMO_RGB_MAX_IMAGE_PIXELS");
  if ((long long)N * H * W > CAMO_RGB_MAX_PIXELS) return fail(CAMO_E_ARG, "N * H * W exceeds CAMO_RGB_MAX_PIXELS");
  return 0;
}
int rg_maps_pointers(const int32_t* segments, const int32_t* region_map, const int32_t* node_off, const uint8_t* gt_mask) {
  if (!segments) return fail(CAMO_E_ARG, "segments is null");
  if (!region_map) return fail(CAMO_E_ARG, "region_map is null");
  if (!node_off) return fail(CAMO_E_ARG, "node_off is null");
  if (!gt_mask) return fail(CAMO_E_ARG, "gt_mask is null");
  return 0;
}
}  // namespace

extern "C" {

int camo_rg_build_csr(const int64_t* edge_index, const float* edge_weight, int32_t N, int32_t E, int32_t* scratch, int32_t* rowptr,
                      int32_t* col, float* w, void* stream) {
  if (N < 1 || E < 0 || (E > 0 && !edge_index) || !scratch || !rowptr || !col || !w) return fail(CAMO_E_ARG, "bad build_csr arguments");
  // scratch: 3 N words = counts | cursor | self-loop weights
  CK(launch_build_csr(reinterpret_cast<const long long*>(edge_index), reinterpret_cast<const long long*>(edge_index) + E, edge_weight, N, E,
                      scratch, reinterpret_cast<float*>(scratch + 2 * (size_t)N), scratch + N, rowptr, col, w, static_cast<hipStream_t>(stream)),
     "build csr");
  return 0;
}

size_t camo_rg_workspace_bytes(const camo_rg_dims_t* dims, int32_t N) {
  if (rg_check(dims, N)) return 0;
  return rg_carve(*dims, N, nullptr).bytes;
}

int camo_rg_node_embeddings(const camo_rg_dims_t* dims, const float* const* params, const float* x, const int32_t* rowptr,
                            const int32_t* col, const float* w, int32_t N, int32_t E, void* workspace, size_t workspace_bytes,
                            float* out, void* stream) {
  if (int e = rg_check(dims, N)) return e;
  if (!params || !x || !rowptr || !col || !w || !workspace || !out || E < N) return fail(CAMO_E_ARG, "null pointer argument or E < N (one self-loop per node)");
  const camo_rg_dims_t& d = *dims;
  const RgWs ws = rg_carve(d, N, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_rg_workspace_bytes()");
  return rg_forward(d, params, x, rowptr, col, w, N, ws, out, static_cast<hipStream_t>(stream));
}

size_t camo_rg_graph_workspace_bytes(int32_t n_labels) {
  if (n_labels < 1 || n_labels > CAMO_RG_MAX_LABELS) return 0;
  return rg_graph_carve(n_labels, nullptr).bytes;
}

int camo_rg_region_graph(const float* image, const int32_t* segments, const uint8_t* canny, int32_t H, int32_t W, int32_t n_labels,
                         void* workspace, size_t workspace_bytes, float* x, int32_t* region_map, int64_t* edge_index,
                         float* edge_attr, int32_t edge_capacity, int32_t* counts, void* stream) {
  if (!image || !segments || !canny || !workspace || !x || !region_map || !edge_index || !edge_attr || !counts)
    return fail(CAMO_E_ARG, "null pointer argument");
  if (H < 1 || W < 1 || (long long)H * W > (1ll << 26)) return fail(CAMO_E_ARG, "image size out of range");
  if (n_labels < 1 || n_labels > CAMO_RG_MAX_LABELS) return fail(CAMO_E_ARG, "n_labels must be in [1, 4096]");
  if (edge_capacity < 2) return fail(CAMO_E_ARG, "edge_capacity must be >= 2");
  const RgGraphWs ws = rg_graph_carve(n_labels, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_rg_graph_workspace_bytes()");
  CK(launch_region_graph(image, segments, canny, H, W, n_labels, ws, x, region_map, reinterpret_cast<long long*>(edge_index), edge_attr,
                         edge_capacity, counts, static_cast<hipStream_t>(stream)), "region graph");
  return 0;
}

static_assert(RGB_SLOTS == CAMO_RGB_TILE_SLOTS && RGB_FIX_BITS == CAMO_RGB_FIX_BITS, "include/camo_rg_batch.h states the kernel's constants");

static int rg_batch_check(int N, int H, int W, int label_bound) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if (N > CAMO_RGB_MAX_IMAGES) return fail(CAMO_E_UNSUPPORTED, "N exceeds CAMO_RGB_MAX_IMAGES");
  if ((long long)H * W > CAMO_RGB_MAX_IMAGE_PIXELS)
    return fail(CAMO_E_UNSUPPORTED, "H * W exceeds CAMO_RGB_MAX_IMAGE_PIXELS (the 64-bit fixed-point sums hold 2^26 pixels)");
  if ((long long)N * H * W > CAMO_RGB_MAX_PIXELS) return fail(CAMO_E_UNSUPPORTED, "N * H * W exceeds CAMO_RGB_MAX_PIXELS (32-bit edge offsets)");
  if (label_bound < 1 || label_bound > CAMO_RG_MAX_LABELS) return fail(CAMO_E_ARG, "label_bound must be in [1, 4096]");
  return 0;
}

size_t camo_rg_batch_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t label_bound) {
  if (rg_batch_check(N, H, W, label_bound)) return 0;
  return rg_batch_carve(N, label_bound, nullptr).bytes;
}

int camo_rg_region_graph_batch(const float* images, const int32_t* segments, const uint8_t* canny, int32_t N, int32_t H, int32_t W,
                               int32_t label_bound, void* workspace, size_t workspace_bytes, float* x, int32_t node_capacity,
                               int32_t* region_map, int64_t* edge_index, float* edge_attr, int32_t edge_capacity, int32_t* node_off,
                               int32_t* edge_off, int32_t* batch, int32_t* status, void* stream) {
  if (int e = rg_batch_check(N, H, W, label_bound)) return e;
  if ((long long)node_capacity < (long long)N * label_bound) return fail(CAMO_E_ARG, "node_capacity must be >= N * label_bound");
  if (edge_capacity < 2) return fail(CAMO_E_ARG, "edge_capacity must be >= 2");
  const RgBatchWs ws = rg_batch_carve(N, label_bound, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_rg_batch_workspace_bytes()");
  if (!images || !segments || !canny || !workspace || !x || !region_map || !edge_index || !edge_attr || !node_off || !edge_off || !batch || !status)
    return fail(CAMO_E_ARG, "null pointer argument");
  CK(launch_region_graph_batch(images, segments, canny, N, H, W, label_bound, ws, x, region_map, reinterpret_cast<long long*>(edge_index),
                               edge_attr, edge_capacity, node_off, edge_off, batch, status, static_cast<hipStream_t>(stream)),
     "region graph batch");
  return 0;
}

// taps->w = the normalised Gaussian of `sigma` at -radius .. radius (sums in double, rounded to float once), radius >= 1
static void gaussian_taps(float sigma, int radius, CannyTaps* taps) {
  *taps = CannyTaps{};
  taps->radius = radius;
  double phi[2 * CANNY_MAX_RADIUS + 1], sum = 0.0;
  for (int k = -radius; k <= radius; ++k) sum += phi[k + radius] = std::exp(-0.5 / ((double)sigma * sigma) * k * k);
  for (int k = 0; k <= 2 * radius; ++k) taps->w[k] = (float)(phi[k] / sum);
}

static int canny_check(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if ((long long)N * H * W > CAMO_CANNY_MAX_PIXELS) return fail(CAMO_E_UNSUPPORTED, "N * H * W exceeds CAMO_CANNY_MAX_PIXELS (32-bit pixel indices)");
  return 0;
}

size_t camo_canny_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (canny_check(N, H, W)) return 0;
  return canny_carve((size_t)N * H * W, nullptr).bytes;
}

int camo_canny(const float* images, int32_t N, int32_t H, int32_t W, float sigma, float low, float high, void* workspace,
               size_t workspace_bytes, uint8_t* edges, float* grad, void* stream) {
  if (int e = canny_check(N, H, W)) return e;
  if (!(sigma > 0.f)) return fail(CAMO_E_ARG, "sigma must be > 0");
  if (!(low > 0.f && low <= high)) return fail(CAMO_E_ARG, "need 0 < low <= high");
  if (!images || !workspace || !edges) return fail(CAMO_E_ARG, "null pointer argument");
  const double radius = 4.0 * (double)sigma + 0.5;
  if (!(radius < CAMO_CANNY_MAX_RADIUS + 1)) return fail(CAMO_E_UNSUPPORTED, "the blur radius int(4 sigma + 0.5) must be <= 32");
  const CannyWs ws = canny_carve((size_t)N * H * W, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_canny_workspace_bytes()");
  CannyTaps taps;
  gaussian_taps(sigma, (int)radius, &taps);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* g = grad ? grad : ws.grad;
  CK(launch_canny_gradients(images, N, H, W, taps, g, st), "canny gradients");
  CK(launch_canny_hysteresis(g, nullptr, low, high, N, H, W, ws, edges, st), "canny hysteresis");
  return 0;
}

int camo_canny_hysteresis(const uint8_t* cls, int32_t N, int32_t H, int32_t W, void* workspace, size_t workspace_bytes, uint8_t* edges,
                          void* stream) {
  if (int e = canny_check(N, H, W)) return e;
  if (!cls || !workspace || !edges) return fail(CAMO_E_ARG, "null pointer argument");
  const CannyWs ws = canny_carve((size_t)N * H * W, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_canny_workspace_bytes()");
  CK(launch_canny_hysteresis(nullptr, cls, 0.f, 0.f, N, H, W, ws, edges, static_cast<hipStream_t>(stream)), "canny hysteresis");
  return 0;
}

// include/camo_slic.h step 4
static int slic_grid(int H, int W, int n_segments, SlicGrid* g) {
  if (H < 1 || W < 1 || n_segments < 1) return fail(CAMO_E_ARG, "need H >= 1, W >= 1, n_segments >= 1");
  const long long hw = (long long)H * W;
  if (hw > CAMO_SLIC_MAX_IMAGE_PIXELS) return fail(CAMO_E_UNSUPPORTED, "H * W exceeds CAMO_SLIC_MAX_IMAGE_PIXELS");
  if (hw <= n_segments) return fail(CAMO_E_UNSUPPORTED, "need H * W > n_segments");
  const double s = std::sqrt((double)hw / n_segments);
  if ((double)std::min(H, W) < s) return fail(CAMO_E_UNSUPPORTED, "need min(H, W) >= sqrt(H * W / n_segments)");
  g->step = (int)std::nearbyint(s);                                         // (round-half-even in the default rounding mode)
  g->start = (int)std::floor(s / 2);
  g->ny = (H - g->start + g->step - 1) / g->step;
  g->nx = (W - g->start + g->step - 1) / g->step;
  const long long K = (long long)g->ny * g->nx;
  if (K > CAMO_RG_MAX_LABELS - 1) return fail(CAMO_E_UNSUPPORTED, "the grid has more than CAMO_RG_MAX_LABELS - 1 centroids");
  g->K = (int)K;
  return 0;
}

static int slic_check(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if (N > CAMO_SLIC_MAX_IMAGES) return fail(CAMO_E_UNSUPPORTED, "N exceeds CAMO_SLIC_MAX_IMAGES");
  if ((long long)H * W > CAMO_SLIC_MAX_IMAGE_PIXELS) return fail(CAMO_E_UNSUPPORTED, "H * W exceeds CAMO_SLIC_MAX_IMAGE_PIXELS");
  if ((long long)N * H * W > CAMO_SLIC_MAX_PIXELS) return fail(CAMO_E_UNSUPPORTED, "N * H * W exceeds CAMO_SLIC_MAX_PIXELS (32-bit pixel indices)");
  return 0;
}

static int slic_taps(float compactness, float sigma, CannyTaps* taps) {
  if (!(compactness >= CAMO_SLIC_MIN_COMPACTNESS) || !std::isfinite(compactness))
    return fail(compactness > 0.f ? CAMO_E_UNSUPPORTED : CAMO_E_ARG, "compactness must be finite and >= CAMO_SLIC_MIN_COMPACTNESS");
  if (!(sigma >= 0.f)) return fail(CAMO_E_ARG, "sigma must be >= 0");
  const double radius = 4.0 * (double)sigma + 0.5;
  if (!(radius < CAMO_SLIC_MAX_RADIUS + 1)) return fail(CAMO_E_UNSUPPORTED, "the blur radius int(4 sigma + 0.5) must be <= 32");
  if ((int)radius == 0) { *taps = CannyTaps{}; taps->w[0] = 1.f; return 0; }       // no blur: the identity tap
  gaussian_taps(sigma, (int)radius, taps);
  return 0;
}

int camo_slic_grid(int32_t H, int32_t W, int32_t n_segments, int32_t* out) {
  if (!out) return fail(CAMO_E_ARG, "null pointer argument");
  SlicGrid g{};
  if (int e = slic_grid(H, W, n_segments, &g)) return e;
  out[0] = g.K; out[1] = g.step; out[2] = g.start; out[3] = g.ny; out[4] = g.nx;
  return 0;
}

size_t camo_slic_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t n_segments) {
  if (slic_check(N, H, W)) return 0;
  if (n_segments == 0) return slic_conn_carve(N, H, W, nullptr).bytes;
  SlicGrid g{};
  if (slic_grid(H, W, n_segments, &g)) return 0;
  return slic_carve(N, H, W, g.K, nullptr).bytes;
}

int camo_slic(const float* images, int32_t N, int32_t H, int32_t W, int32_t n_segments, float compactness, float sigma, void* workspace,
              size_t workspace_bytes, int32_t* labels, int32_t* counts, void* stream) {
  if (int e = slic_check(N, H, W)) return e;
  SlicGrid g{};
  if (int e = slic_grid(H, W, n_segments, &g)) return e;
  CannyTaps taps;
  if (int e = slic_taps(compactness, sigma, &taps)) return e;
  if (!images || !workspace || !labels || !counts) return fail(CAMO_E_ARG, "null pointer argument");
  const SlicWs ws = slic_carve(N, H, W, g.K, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_slic_workspace_bytes()");
  hipStream_t st = static_cast<hipStream_t>(stream);
  CK(launch_slic_preprocess(images, N, H, W, taps, 1.0f / compactness, ws.lab, st), "slic preprocess");
  CK(launch_slic_init(g, N, ws.cent, ws.sums, st), "slic init");
  for (int it = 0; it < SLIC_ITERATIONS; ++it) {
    CK(launch_slic_assign(ws.lab, ws.cent, N, H, W, g.K, g.step, ws.nearest, nullptr, st), "slic assign");
    if (it + 1 < SLIC_ITERATIONS) CK(launch_slic_update(ws.lab, ws.nearest, N, H, W, g.K, ws.sums, ws.cent, false, st), "slic update");
  }
  // (connected components of equal labels: the "+ 1" of step 7 changes none of them)
  const double segment = (double)H * W / g.K;
  CK(launch_slic_connect(ws.nearest, N, H, W, (int)(0.5 * segment), (int)(3.0 * segment), ws.conn, labels, counts, st), "slic connect");
  return 0;
}

int camo_slic_preprocess(const float* images, int32_t N, int32_t H, int32_t W, float compactness, float sigma, float* lab, void* stream) {
  if (int e = slic_check(N, H, W)) return e;
  CannyTaps taps;
  if (int e = slic_taps(compactness, sigma, &taps)) return e;
  if (!images || !lab) return fail(CAMO_E_ARG, "null pointer argument");
  CK(launch_slic_preprocess(images, N, H, W, taps, 1.0f / compactness, lab, static_cast<hipStream_t>(stream)), "slic preprocess");
  return 0;
}

static int slic_k_check(int K, int step) {
  if (K < 1 || K > CAMO_RG_MAX_LABELS - 1) return fail(CAMO_E_ARG, "K must be in [1, CAMO_RG_MAX_LABELS - 1]");
  if (step < 1 || step > 4096) return fail(CAMO_E_ARG, "step must be in [1, 4096]");
  return 0;
}

int camo_slic_assign(const float* lab, const float* centroids, int32_t N, int32_t H, int32_t W, int32_t K, int32_t step, int32_t* nearest,
                     float* dist, void* stream) {
  if (int e = slic_check(N, H, W)) return e;
  if (int e = slic_k_check(K, step)) return e;
  if (!lab || !centroids || !nearest || !dist) return fail(CAMO_E_ARG, "null pointer argument");
  CK(launch_slic_assign(lab, centroids, N, H, W, K, step, nearest, dist, static_cast<hipStream_t>(stream)), "slic assign");
  return 0;
}

int camo_slic_update(const float* lab, const int32_t* nearest, int32_t N, int32_t H, int32_t W, int32_t K, int64_t* sums, float* centroids,
                     void* stream) {
  if (int e = slic_check(N, H, W)) return e;
  if (int e = slic_k_check(K, 1)) return e;
  if (!lab || !nearest || !sums || !centroids) return fail(CAMO_E_ARG, "null pointer argument");
  CK(launch_slic_update(lab, nearest, N, H, W, K, reinterpret_cast<long long*>(sums), centroids, true, static_cast<hipStream_t>(stream)),
     "slic update");
  return 0;
}

int camo_slic_connect(const int32_t* labels_in, int32_t N, int32_t H, int32_t W, int32_t min_size, int32_t max_size, void* workspace,
                      size_t workspace_bytes, int32_t* labels, int32_t* counts, void* stream) {
  if (int e = slic_check(N, H, W)) return e;
  if (min_size < 0 || max_size < 1) return fail(CAMO_E_ARG, "need min_size >= 0 and max_size >= 1");
  if (!labels_in || !workspace || !labels || !counts) return fail(CAMO_E_ARG, "null pointer argument");
  const SlicConnWs ws = slic_conn_carve(N, H, W, workspace);
  if (workspace_bytes < ws.bytes) return fail(CAMO_E_WORKSPACE, "workspace smaller than camo_slic_workspace_bytes(N, H, W, 0)");
  CK(launch_slic_connect(labels_in, N, H, W, min_size, max_size, ws, labels, counts, static_cast<hipStream_t>(stream)), "slic connect");
  return 0;
}

static_assert(CAMO_RGD_NPARAMS == 12 && CAMO_RGD_MAX_CLASSES == 8, "rg_detect.h sizes its parameter table and its logit rows by these");

int camo_rg_node_heads(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* head_params, const float* emb, int32_t n,
                       float* logits, float* probs, void* stream) {
  if (!dims) return fail(CAMO_E_ARG, "dims is null");
  if (dims->hidden < 2 || dims->hidden > CAMO_RGD_MAX_HIDDEN || (dims->hidden & 1))
    return fail(CAMO_E_ARG, "hidden must be even and in [2, CAMO_RGD_MAX_HIDDEN]");
  if (num_classes < 2 || num_classes > CAMO_RGD_MAX_CLASSES) return fail(CAMO_E_ARG, "num_classes must be in [2, CAMO_RGD_MAX_CLASSES]");
  if (n < 1) return fail(CAMO_E_ARG, "need n >= 1");
  if (!head_params || !emb || !logits || !probs) return fail(CAMO_E_ARG, "null pointer argument");
  RgdHeads P{};
  for (int i = 0; i < CAMO_RGD_NPARAMS; ++i) {
    if (!head_params[i]) return fail(CAMO_E_ARG, "null pointer in the head parameter table");
    P.p[i] = head_params[i];
  }
  CK(launch_rgd_heads(P, emb, n, dims->hidden, num_classes, logits, probs, static_cast<hipStream_t>(stream)), "rg node heads");
  return 0;
}

int camo_rg_paint(const float* values, int32_t n_nodes, int32_t C, const int32_t* segments, const int32_t* region_map,
                  const int32_t* node_off, int32_t N, int32_t H, int32_t W, int32_t label_bound, float fill, float* maps, void* stream) {
  if (C < 1 || C > CAMO_RGD_MAX_CHANNELS) return fail(CAMO_E_ARG, "C must be in [1, CAMO_RGD_MAX_CHANNELS]");
  if (n_nodes < 1 || N < 1 || H < 1 || W < 1 || label_bound < 1) return fail(CAMO_E_ARG, "need n_nodes >= 1, N >= 1, H >= 1, W >= 1, label_bound >= 1");
  if ((long long)N * H * W > CAMO_RGD_MAX_PIXELS) return fail(CAMO_E_ARG, "N * H * W exceeds CAMO_RGD_MAX_PIXELS");
  if (!values || !segments || !region_map || !node_off || !maps) return fail(CAMO_E_ARG, "null pointer argument");
  CK(launch_rgd_paint(values, n_nodes, C, segments, region_map, node_off, N, H, W, label_bound, fill, maps, static_cast<hipStream_t>(stream)),
     "rg paint");
  return 0;
}

int camo_seg_counts(const float* pred, int64_t pred_image_stride, const uint8_t* gt, float threshold, int32_t N, int32_t H, int32_t W,
                    int64_t* counts, void* stream) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if (N > CAMO_RGD_MAX_IMAGES) return fail(CAMO_E_ARG, "N exceeds CAMO_RGD_MAX_IMAGES");
  if ((long long)H * W > CAMO_RGD_MAX_IMAGE_PIXELS) return fail(CAMO_E_ARG, "H * W exceeds CAMO_RGD_MAX_IMAGE_PIXELS (the integer absolute-error sum holds 2^26 pixels)");
  if (pred_image_stride < (long long)H * W) return fail(CAMO_E_ARG, "pred_image_stride must be >= H * W");
  if (threshold != threshold) return fail(CAMO_E_ARG, "threshold is NaN");
  if (!pred || !gt || !counts) return fail(CAMO_E_ARG, "null pointer argument");
  CK(launch_rgd_counts(pred, pred_image_stride, gt, threshold, N, H, W, reinterpret_cast<unsigned long long*>(counts),
                       static_cast<hipStream_t>(stream)), "seg counts");
  return 0;
}

// ---- Region-graph GNN loss and gradients, batch norm frozen (include/camo_rg_train.h) --------------------------
static_assert(CAMO_RGT_NGRADS == 32 && CAMO_RGT_FC_B == 19 && CAMO_RGT_HEADS == 20, "the gradient table is the 20 + 12 trainable parameters");

size_t camo_rg_train_workspace_bytes(const camo_rg_dims_t* dims, int32_t num_classes, int32_t N, int32_t E) {
  return rgt_workspace_bytes(dims, num_classes, N, E, false);
}

// The one launch sequence of all four entries.  batch: null = frozen statistics (camo_rg_loss_backward), else the batch-statistics mode
// (its stats and partial are filled in here from the workspace).  drop: null = no dropout, else include/camo_rg_train_drop.h -- the
// forward's eight sites, and in the backward nothing but a scale: every ReLU mask is taken from the saved, dropped activation, which
// is > 0 exactly where the element was kept and the ReLU is open, so the mask's 1 becomes 1 / (1 - p).  pixel: null = the sequence
// without it launch for launch, else include/camo_rg_pixel_loss.h -- two launches right after the loss, which add the pixel term to
// dlogits and to the loss figures (loss is float[6] then); the backward that follows does not know.
static int rgt_run(const RgtCall& c, RgBatchNorm* batch, const RgDropout* drop, const RgPixel* pixel) {
  const int N = c.N, nc = c.num_classes;
  if (int e = rgt_check(c.dims, nc, N, c.E, batch != nullptr)) return e;
  if (!c.params || !c.head_params || !c.x || !c.rowptr || !c.col || !c.w || !c.rrowptr || !c.rcol || !c.rw || !c.mask_t || !c.inst_t ||
      !c.edge_t || !c.workspace || !c.loss || !c.grads)
    return fail(CAMO_E_ARG, "null pointer argument");
  for (int i = 0; i < CAMO_RG_NPARAMS; ++i)
    if (!c.params[i] && !(batch && rg_running_slot(i))) return fail(CAMO_E_ARG, "null pointer in the parameter table");
  for (int i = 0; i < CAMO_RGD_NPARAMS; ++i)
    if (!c.head_params[i]) return fail(CAMO_E_ARG, "null pointer in the head parameter table");
  for (int i = 0; i < CAMO_RGT_NGRADS; ++i)
    if (!c.grads[i]) return fail(CAMO_E_ARG, "null pointer in the gradient table");
  if (!std::isfinite(c.w_mask) || !std::isfinite(c.w_instance) || !std::isfinite(c.w_edge)) return fail(CAMO_E_ARG, "loss weights must be finite");
  if (batch && batch->running) {
    for (int i = 0; i < 8; ++i)
      if (!batch->running[i]) return fail(CAMO_E_ARG, "null pointer in the running-statistics table");
    if (!std::isfinite(batch->momentum) || !(batch->momentum > 0.f && batch->momentum <= 1.f))
      return fail(CAMO_E_ARG, "momentum must be finite and in (0, 1] when running is given");
  }
  const camo_rg_dims_t& d = *c.dims;
  const RgtWs ws = rgt_carve(d, nc, N, c.workspace, batch != nullptr);
  if (c.workspace_bytes < ws.bytes)
    return fail(CAMO_E_WORKSPACE, batch ? "workspace smaller than camo_rg_train_bn_workspace_bytes()" : "workspace smaller than camo_rg_train_workspace_bytes()");
  if (batch) { batch->stats = ws.stats; batch->partial = ws.partial; }
  const bool bs = batch != nullptr;
  hipStream_t st = static_cast<hipStream_t>(c.stream);
  const int C = d.hidden, K = d.heads, In = d.in_channels, Hh = C / 2, units = 3 * Hh, L = 2 * nc + 1;
  const int nb = rgt_row_blocks(N);
  const float* const* P = c.params;
  const float* const* HP = c.head_params;
  float* const* G = c.grads;
  float* const* GH = c.grads + CAMO_RGT_HEADS;
  auto bn = [&](int slot) { return BnEval{P[slot], P[slot + 1], P[slot + 2], P[slot + 3]}; };
  // dy (ReLU-masked, in dB) -> the layer's batch-norm gradients, its conv-bias gradient, and dPre in place.  Frozen: dPre = dy weight /
  // sqrt(var + eps), scaled by the first launch.  Batch statistics: the sums first, then dz from the finished sums (a third launch).
  auto bn_backward = [&](int layer, int slot, float* dweight, float* dbias_bn, float* dbias_conv) -> int {
    CK(launch_rgt_bn_backward(ws.dB, ws.xhat[layer], bn(slot), N, C, ws.partial, st, bs), "bn backward");
    CK(launch_rgt_bn_finish(ws.partial, nb, bn(slot), C, dweight, dbias_bn, dbias_conv, st, bs), "bn gradients");
    if (bs) CK(launch_rgt_bn_dz(ws.dB, ws.xhat[layer], P[slot], ws.stats + (size_t)layer * 2 * C + C, dweight, dbias_bn, N, C, st), "bn input gradient");
    return 0;
  };
  constexpr int KM = GF_A_KMAJOR | GF_B_KMAJOR;   // dW = dY^T . X without atomics: one block owns an output tile over the whole contraction
  const bool dhead = drop && drop->head.p > 0.f;
  const float s_conv = drop ? drop->conv.scale : 1.f, s_shared = drop ? drop->shared.scale : 1.f, s_head = drop ? drop->head.scale : 1.f;
  GB g(dhead ? drop->head : make_drop(0, 0.f, 0), CAMO_PREC_F32, st);   // (only the heads' first layers carry GF_DROPOUT in this batch)

  // ---- forward, saving (camo_rg_node_embeddings + camo_rg_node_heads) ----
  if (int e = rg_forward(d, P, c.x, c.rowptr, c.col, c.w, N, ws, ws.emb, st, batch, drop)) return e;
  CK(launch_rgt_concat_heads(HP, ws.W1, ws.b1, C, st), "head weights");
  g.nt(ws.emb, C, ws.W1, C, ws.b1, ws.Z, units, N, units, C, dhead ? GF_RELU | GF_DROPOUT : GF_RELU).drop_site = SITE_RGT_HEADS;
  CK(g.run(), "head first layers");
  CK(launch_rgt_head_logits(HP, ws.Z, ws.logits, N, C, nc, st), "head logits");

  // ---- loss and dlogits ----
  CK(launch_rgt_loss(ws.logits, c.mask_t, c.inst_t, c.edge_t, c.w_mask, c.w_instance, c.w_edge, N, nc, c.loss, ws.dlogits, st), "loss");
  if (pixel) CK(launch_rgt_pixel_loss(ws.logits, *pixel, N, nc, c.loss, ws.dlogits, st), "pixel loss");

  // ---- heads backward ----
  CK(launch_rgt_cross_partial(nullptr, 0, 1, ws.dlogits, L, L, N, ws.partial, st), "head bias sums");
  CK(launch_rgt_colsum_finish(ws.partial, nb, L, RgtSegs{{GH[CAMO_RGD_MASK_B2], GH[CAMO_RGD_INST_B2], GH[CAMO_RGD_EDGE_B2], nullptr},
                                                         {0, nc, 2 * nc, L, L}, 3}, st), "head bias sums");
  for (int h = 0; h < 3; ++h) {
    const int nch = h < 2 ? nc : 1;
    CK(launch_rgt_cross_partial(ws.dlogits + h * nc, L, nch, ws.Z + h * Hh, units, Hh, N, ws.partial, st), "head second-layer gradient");
    CK(launch_rgt_colsum_finish(ws.partial, nb, nch * Hh, RgtSegs{{GH[4 * h + 2], nullptr, nullptr, nullptr}, {0, nch * Hh, 0, 0, 0}, 1}, st),
       "head second-layer gradient");
  }
  CK(launch_rgt_head_dz(HP, ws.Z, ws.dlogits, ws.dZ, N, C, nc, st, s_head), "head hidden gradient");
  CK(launch_rgt_cross_partial(nullptr, 0, 1, ws.dZ, units, units, N, ws.partial, st), "head first-layer bias sums");
  CK(launch_rgt_colsum_finish(ws.partial, nb, units, RgtSegs{{GH[CAMO_RGD_MASK_B1], GH[CAMO_RGD_INST_B1], GH[CAMO_RGD_EDGE_B1], nullptr},
                                                             {0, Hh, 2 * Hh, units, units}, 3}, st), "head first-layer bias sums");
  for (int h = 0; h < 3; ++h) g.add(ws.dZ + h * Hh, units, ws.emb, C, GH[4 * h], C, Hh, C, N, KM);
  set_relu_bwd(g.nn(ws.dZ, units, ws.W1, C, ws.dA, C, N, C, units), ws.emb, C, s_shared);            // dA = d(fc_shared pre-activation)
  CK(g.run(), "head first-layer gradients");

  // ---- fc_shared backward ----
  CK(launch_rgt_cross_partial(nullptr, 0, 1, ws.dA, C, C, N, ws.partial, st), "fc_shared bias sums");
  CK(launch_rgt_colsum_finish(ws.partial, nb, C, RgtSegs{{G[CAMO_RGT_FC_B], nullptr, nullptr, nullptr}, {0, C, 0, 0, 0}, 1}, st), "fc_shared bias sums");
  g.add(ws.dA, C, ws.h[3], C, G[CAMO_RGT_FC_W], C, C, C, N, KM);
  set_relu_bwd(g.nn(ws.dA, C, P[CAMO_RG_FC_W], C, ws.dB, C, N, C, C), ws.h[3], C, s_conv);           // dB = dy of bn4 (ReLU-masked)
  CK(g.run(), "fc_shared gradients");

  // ---- conv4 .. conv2 backward: dB = dy -> dPre (in place) -> dA = dXW -> dB = dy of the layer below ----
  for (int k = 2; k >= 0; --k) {
    const int base = CAMO_RG_C2_BIAS + 6 * k, gb = CAMO_RGT_C2_BIAS + 4 * k;
    if (int e = bn_backward(k + 1, base + 2, G[gb + 2], G[gb + 3], G[gb])) return e;
    CK(launch_rgt_gcn_backward(ws.dB, c.rrowptr, c.rcol, c.rw, ws.dinv, ws.dA, N, C, st), "gcn aggregate backward");
    g.add(ws.dA, C, ws.h[k], C, G[gb + 1], C, C, C, N, KM);
    set_relu_bwd(g.nn(ws.dA, C, P[base + 1], C, ws.dB, C, N, C, C), ws.h[k], C, s_conv);
    CK(g.run(), "gcn projection gradients");
  }

  // ---- conv1 (GAT) backward ----
  if (int e = bn_backward(0, CAMO_RG_BN1, G[CAMO_RGT_BN1_W], G[CAMO_RGT_BN1_B], G[CAMO_RGT_C1_BIAS])) return e;
  CK(launch_rgt_gat_backward_a(ws.dB, ws.Hh, ws.O, ws.a_src, ws.a_dst, ws.m, ws.S, c.rowptr, c.col, ws.r, ws.da_dst, N, K, C, st), "gat backward A");
  CK(launch_rgt_gat_backward_b(ws.dB, ws.Hh, ws.a_src, ws.a_dst, ws.m, ws.S, ws.r, ws.da_dst, P[CAMO_RG_C1_ATT_SRC], P[CAMO_RG_C1_ATT_DST],
                               c.rrowptr, c.rcol, ws.da_src, ws.dh, N, K, C, st), "gat backward B");
  CK(launch_rgt_att_partial(ws.da_src, ws.da_dst, ws.Hh, N, K, C, ws.partial, st), "attention vector sums");
  CK(launch_rgt_colsum_finish(ws.partial, nb, 2 * K * C, RgtSegs{{G[CAMO_RGT_C1_ATT_SRC], G[CAMO_RGT_C1_ATT_DST], nullptr, nullptr},
                                                                 {0, K * C, 2 * K * C, 0, 0}, 2}, st), "attention vector sums");
  g.add(ws.dh, K * C, c.x, In, G[CAMO_RGT_C1_W], In, K * C, In, N, KM);
  CK(g.run(), "gat projection gradient");
  return 0;
}

int camo_rg_loss_backward(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                          const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                          const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                          const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                          float* loss, float* const* grads, void* stream) {
  const RgtCall c{dims, num_classes, params, head_params, x, rowptr, col, w, rrowptr, rcol, rw, N, E, mask_t, inst_t, edge_t, w_mask, w_instance,
                  w_edge, workspace, workspace_bytes, loss, grads, stream};
  return rgt_run(c, nullptr, nullptr, nullptr);
}

// ---- The same with batch-statistics batch norm (include/camo_rg_train_bn.h) --------------------------------------
size_t camo_rg_train_bn_workspace_bytes(const camo_rg_dims_t* dims, int32_t num_classes, int32_t N, int32_t E) {
  return rgt_workspace_bytes(dims, num_classes, N, E, true);
}

int camo_rg_loss_backward_bn(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                             const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                             const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                             const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                             float* loss, float* const* grads, float momentum, float* const* running, float* batch_stats, void* stream) {
  const RgtCall c{dims, num_classes, params, head_params, x, rowptr, col, w, rrowptr, rcol, rw, N, E, mask_t, inst_t, edge_t, w_mask, w_instance,
                  w_edge, workspace, workspace_bytes, loss, grads, stream};
  RgBatchNorm batch{nullptr, nullptr, running, momentum, batch_stats};
  return rgt_run(c, &batch, nullptr, nullptr);
}

// ---- The same with dropout, in either batch-norm mode (include/camo_rg_train_drop.h) ----------------------------------
static_assert(CAMO_RGT_SITE_CONV0 == SITE_RGT_CONV0 && CAMO_RGT_SITE_SHARED == SITE_RGT_SHARED && CAMO_RGT_SITE_HEADS == SITE_RGT_HEADS &&
              SITE_RGT_CONV0 > SITE_LATE0 + 1 && SITE_RGT_CONV0 + 4 == SITE_RGT_SHARED, "the header states common.h's site numbers; the fusion sites end at 11");

size_t camo_rg_train_drop_workspace_bytes(const camo_rg_dims_t* dims, int32_t num_classes, int32_t N, int32_t E, int32_t batch_stats) {
  return rgt_workspace_bytes(dims, num_classes, N, E, batch_stats != 0);
}

// camo_rg_loss_backward_drop, and camo_rg_loss_backward_pixel (include/camo_rg_pixel_loss.h) once it has checked its own arguments
static int rgt_run_drop(const RgtCall& c, float momentum, float* const* running, float* batch_stats, int32_t batch_stats_mode, float p_conv,
                        float p_shared, float p_head, uint64_t seed, const RgPixel* pixel) {
  if (batch_stats_mode != 0 && batch_stats_mode != 1) return fail(CAMO_E_ARG, "batch_stats_mode must be 0 (frozen statistics) or 1 (batch statistics)");
  for (float p : {p_conv, p_shared, p_head})
    if (!std::isfinite(p) || !(p >= 0.f && p < 1.f)) return fail(CAMO_E_ARG, "dropout rates must be finite and in [0, 1)");
  if (batch_stats_mode == 0 && (running || batch_stats))
    return fail(CAMO_E_ARG, "running and batch_stats must be null in batch_stats_mode 0 (frozen statistics)");
  if (c.dims && c.N >= 1 && c.dims->hidden >= 2 && (long long)c.N * (3 * (c.dims->hidden / 2)) >= (1ll << 32))
    return fail(CAMO_E_UNSUPPORTED, "N * (3 hidden / 2) must be < 2^32 (32-bit dropout element indices)");
  RgBatchNorm batch{nullptr, nullptr, running, momentum, batch_stats};
  const RgDropout drop{make_drop(1, p_conv, seed), make_drop(1, p_shared, seed), make_drop(1, p_head, seed)};
  const bool any = p_conv > 0.f || p_shared > 0.f || p_head > 0.f;      // all zero: the mode's existing entry, launch for launch
  return rgt_run(c, batch_stats_mode ? &batch : nullptr, any ? &drop : nullptr, pixel);
}

int camo_rg_loss_backward_drop(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                               const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                               const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                               const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                               float* loss, float* const* grads, float momentum, float* const* running, float* batch_stats,
                               int32_t batch_stats_mode, float p_conv, float p_shared, float p_head, uint64_t seed, void* stream) {
  const RgtCall c{dims, num_classes, params, head_params, x, rowptr, col, w, rrowptr, rcol, rw, N, E, mask_t, inst_t, edge_t, w_mask, w_instance,
                  w_edge, workspace, workspace_bytes, loss, grads, stream};
  return rgt_run_drop(c, momentum, running, batch_stats, batch_stats_mode, p_conv, p_shared, p_head, seed, nullptr);
}

// ---- The same with the structure loss on the painted mask (include/camo_rg_pixel_loss.h) -----------------------------
static_assert(RGPL_MAX_RADIUS == CAMO_RGPL_MAX_RADIUS && RGPL_MAX_GAIN == CAMO_RGPL_MAX_GAIN, "include/camo_rg_pixel_loss.h states the kernel's constants");

int camo_rg_loss_backward_pixel(const camo_rg_dims_t* dims, int32_t num_classes, const float* const* params, const float* const* head_params,
                                const float* x, const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rrowptr,
                                const int32_t* rcol, const float* rw, int32_t N, int32_t E, const int32_t* mask_t, const int32_t* inst_t,
                                const float* edge_t, float w_mask, float w_instance, float w_edge, void* workspace, size_t workspace_bytes,
                                float* loss, float* const* grads, float momentum, float* const* running, float* batch_stats,
                                int32_t batch_stats_mode, float p_conv, float p_shared, float p_head, uint64_t seed, const int64_t* node_w,
                                const int32_t* node_off, int32_t n_images, int32_t radius, float w_pixel, void* stream) {
  if (num_classes != 2) return fail(CAMO_E_UNSUPPORTED, "the pixel loss needs num_classes == 2 (one logit difference per node)");
  if (n_images < 1) return fail(CAMO_E_ARG, "n_images must be >= 1");
  if (radius < 0 || radius > CAMO_RGPL_MAX_RADIUS) return fail(CAMO_E_ARG, "radius must be in [0, CAMO_RGPL_MAX_RADIUS]");
  if (!std::isfinite(w_pixel) || !(w_pixel >= 0.f)) return fail(CAMO_E_ARG, "w_pixel must be finite and >= 0");
  if (!node_w) return fail(CAMO_E_ARG, "node_w is null");
  if (!node_off) return fail(CAMO_E_ARG, "node_off is null");
  static_assert(sizeof(long long) == sizeof(int64_t), "node_w is int64");
  const RgPixel pixel{reinterpret_cast<const long long*>(node_w), node_off, n_images, radius, w_pixel};
  const RgtCall c{dims, num_classes, params, head_params, x, rowptr, col, w, rrowptr, rcol, rw, N, E, mask_t, inst_t, edge_t, w_mask, w_instance,
                  w_edge, workspace, workspace_bytes, loss, grads, stream};
  return rgt_run_drop(c, momentum, running, batch_stats, batch_stats_mode, p_conv, p_shared, p_head, seed, &pixel);
}

// ---- Node targets from ground-truth masks (include/camo_rg_targets.h) ------------------------------------------
static_assert(RGTG_TILE == CAMO_RGTG_TILE && RGTG_SLOTS == CAMO_RGTG_TILE_SLOTS, "include/camo_rg_targets.h states the kernel's constants");

int camo_rg_node_targets(const int32_t* segments, const int32_t* region_map, const int32_t* node_off, const uint8_t* gt_mask,
                         const uint8_t* gt_instance, const uint8_t* gt_edge, int32_t N, int32_t H, int32_t W, int32_t label_bound,
                         int32_t n_nodes, int32_t band_permille, int32_t edge_min_pixels, int32_t* counts, int32_t* mask_t,
                         int32_t* inst_t, float* edge_t, void* stream) {
  if (int e = rg_maps_sizes(N, H, W, label_bound, n_nodes)) return e;
  if (band_permille < 0 || band_permille >= 500) return fail(CAMO_E_ARG, "band_permille must be in [0, 500)");
  if (edge_min_pixels < 1) return fail(CAMO_E_ARG, "edge_min_pixels must be >= 1");
  if (int e = rg_maps_pointers(segments, region_map, node_off, gt_mask)) return e;
  if (!counts) return fail(CAMO_E_ARG, "counts is null");
  if (!mask_t) return fail(CAMO_E_ARG, "mask_t is null");
  if (!inst_t) return fail(CAMO_E_ARG, "inst_t is null");
  if (!edge_t) return fail(CAMO_E_ARG, "edge_t is null");
  CK(launch_rg_node_targets(segments, region_map, node_off, gt_mask, gt_instance, gt_edge, N, H, W, label_bound, n_nodes, band_permille,
                            edge_min_pixels, counts, mask_t, inst_t, edge_t, static_cast<hipStream_t>(stream)), "rg node targets");
  return 0;
}

// ---- Node weights of the pixel loss from ground-truth masks (include/camo_rg_pixel_loss.h) ----------------------------
int camo_rg_pixel_weights(const int32_t* segments, const int32_t* region_map, const int32_t* node_off, const uint8_t* gt_mask, int32_t N,
                          int32_t H, int32_t W, int32_t label_bound, int32_t n_nodes, int32_t radius, int32_t gain, int64_t* node_w,
                          void* stream) {
  if (int e = rg_maps_sizes(N, H, W, label_bound, n_nodes)) return e;
  if (radius < 0 || radius > CAMO_RGPL_MAX_RADIUS) return fail(CAMO_E_ARG, "radius must be in [0, CAMO_RGPL_MAX_RADIUS]");
  if (gain < 0 || gain > CAMO_RGPL_MAX_GAIN) return fail(CAMO_E_ARG, "gain must be in [0, CAMO_RGPL_MAX_GAIN]");
  if (int e = rg_maps_pointers(segments, region_map, node_off, gt_mask)) return e;
  if (!node_w) return fail(CAMO_E_ARG, "node_w is null");
  CK(launch_rg_pixel_weights(segments, region_map, node_off, gt_mask, N, H, W, label_bound, n_nodes, radius, gain,
                             reinterpret_cast<long long*>(node_w), static_cast<hipStream_t>(stream)), "rg pixel weights");
  return 0;
}
}  // extern "C"
