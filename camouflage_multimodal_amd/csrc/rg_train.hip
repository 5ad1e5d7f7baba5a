// Loss and backward of the region-graph GNN with frozen batch-norm statistics (include/camo_rg_train.h) or with the
// statistics of the call's own nodes (include/camo_rg_train_bn.h); and the structure loss on the painted mask that
// include/camo_rg_pixel_loss.h adds to the loss.
// Like the forward (rg_gnn.hip) the sparse part is latency- and HBM-bound gathers: one wave (GCN) or one block of `heads` waves
// (GAT) per row of a CSR, source rows read as coalesced pieces, CPL channels per lane.  The backward of an aggregation is the same
// gather walked over the REVERSED CSR, so every output row has one owner and no scatter is needed; every column sum over the
// nodes (bias, batch-norm and attention-vector gradients) is per-block partials in row order, then a second stage in block order.
// No floating-point atomic: the gradients are functions of the inputs alone.
#include "rg_train.h"

namespace {

constexpr int NT = 256;

struct HeadPtrs { const float* p[12]; };   // CAMO_RGD_* order

// ---- forward, saving ------------------------------------------------------------------------------------------------------
// grid N, block 64 * heads.  Two walks over the row: the maximum, then the sums (the saved m and S are what the backward
// recomputes alpha from, so they are taken the plain way, not online).  RAW (batch statistics): the pre-activation goes where xhat
// goes; no batch norm, no ReLU, out untouched.  DROP (gat_forward_drop_kernel only, not RAW; include/camo_rg_train_drop.h): inverted
// dropout on out after the ReLU, element index i * C + c; xhat stays undropped.
template <int CPL, bool RAW, bool DROP>
__device__ __forceinline__ void gat_forward_body(const float* __restrict__ Hh, const float* __restrict__ a_src, const float* __restrict__ a_dst,
                                                 const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ bias,
                                                 const BnEval& bn, float* __restrict__ m_out, float* __restrict__ S_out, float* __restrict__ O,
                                                 float* __restrict__ xhat, float* __restrict__ out, int heads, int C, const DropCfg& drop,
                                                 uint32_t site) {
  __shared__ float red[8][64 * CPL];
  const int i = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float ad = a_dst[i * heads + k];
  const int e0 = rowptr[i], e1 = rowptr[i + 1];
  float m = -INFINITY;
  for (int e = e0; e < e1; ++e) m = fmaxf(m, lrelu(a_src[col[e] * heads + k] + ad));
  float s = 0.f, acc[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) acc[q] = 0.f;
  for (int e = e0; e < e1; ++e) {
    const int j = col[e];
    const float p = expf(lrelu(a_src[j * heads + k] + ad) - m);
    s += p;
    const float* h = Hh + ((size_t)j * heads + k) * C;
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < C) acc[q] = fmaf(p, h[c], acc[q]); }
  }
  const float inv = s > 0.f ? 1.0f / s : 0.f;
  float* o = O + ((size_t)i * heads + k) * C;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = lane + 64 * q;
    const float v = acc[q] * inv;
    red[k][c] = v;
    if (c < C) o[c] = v;
  }
  if (lane == 0) { m_out[i * heads + k] = m; S_out[i * heads + k] = s; }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float v = 0.f;
    for (int kk = 0; kk < heads; ++kk) v += red[kk][c];
    if constexpr (RAW) {
      xhat[(size_t)i * C + c] = v / (float)heads + bias[c];
    } else {
      const float xh = bn_xhat(v / (float)heads + bias[c], bn, c);
      xhat[(size_t)i * C + c] = xh;
      float y = bn_relu(xh, bn, c);
      if constexpr (DROP) y *= drop_mult(drop, site, (uint32_t)i * (uint32_t)C + (uint32_t)c);
      out[(size_t)i * C + c] = y;
    }
  }
}

template <int CPL, bool RAW = false>
__global__ void gat_forward_kernel(const float* __restrict__ Hh, const float* __restrict__ a_src, const float* __restrict__ a_dst,
                                   const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ bias, BnEval bn,
                                   float* __restrict__ m_out, float* __restrict__ S_out, float* __restrict__ O, float* __restrict__ xhat,
                                   float* __restrict__ out, int heads, int C) {
  gat_forward_body<CPL, RAW, false>(Hh, a_src, a_dst, rowptr, col, bias, bn, m_out, S_out, O, xhat, out, heads, C, DropCfg{}, 0u);
}

template <int CPL>
__global__ void gat_forward_drop_kernel(const float* __restrict__ Hh, const float* __restrict__ a_src, const float* __restrict__ a_dst,
                                        const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ bias, BnEval bn,
                                        float* __restrict__ m_out, float* __restrict__ S_out, float* __restrict__ O, float* __restrict__ xhat,
                                        float* __restrict__ out, int heads, int C, DropCfg drop, uint32_t site) {
  gat_forward_body<CPL, false, true>(Hh, a_src, a_dst, rowptr, col, bias, bn, m_out, S_out, O, xhat, out, heads, C, drop, site);
}

__global__ void concat_heads_kernel(HeadPtrs P, float* __restrict__ W1, float* __restrict__ b1, int H) {
  const int Hh = H >> 1, units = 3 * Hh;
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx < units * H) {
    const int u = idx / H, k = idx - u * H, h = u / Hh;
    W1[idx] = P.p[4 * h][(size_t)(u - h * Hh) * H + k];
  } else if (idx < units * (H + 1)) {
    const int u = idx - units * H, h = u / Hh;
    b1[u] = P.p[4 * h + 1][u - h * Hh];
  }
}

// one wave per node, 4 nodes per block: logit o = <W2_h[c, :], z_h> + b2_h[c], 64 partial sums of stride 64 added in a fixed tree
__global__ void head_logits_kernel(HeadPtrs P, const float* __restrict__ Z, float* __restrict__ logits, int N, int H, int nc) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const int Hh = H >> 1, L = 2 * nc + 1;
  for (int o = 0; o < L; ++o) {
    const int h = (o >= nc) + (o >= 2 * nc), c = o - h * nc;
    const float* W2 = P.p[4 * h + 2] + (size_t)c * Hh;
    const float* z = Z + (size_t)n * 3 * Hh + h * Hh;
    float s = 0.f;
    for (int j = lane; j < Hh; j += 64) s = fmaf(W2[j], z[j], s);
    s = wave_sum(s);
    if (lane == 0) logits[(size_t)n * L + o] = s + P.p[4 * h + 3][c];
  }
}

// ---- loss -------------------------------------------------------------------------------------------------------------------
// ONE block of 1024 threads.  First the integer counts of the non-ignored nodes, then per node the three terms and dlogits, already
// scaled by weight / count; the sums are per-thread doubles in node order, a butterfly per wave, the 16 waves in order.
__global__ __launch_bounds__(1024) void loss_kernel(const float* __restrict__ logits, const int* __restrict__ mask_t, const int* __restrict__ inst_t,
                                                    const float* __restrict__ edge_t, float wm, float wi, float we, int N, int nc,
                                                    float* __restrict__ loss, float* __restrict__ dlogits) {
  __shared__ int cnt_w[3][16];
  __shared__ double sum_w[3][16];
  __shared__ int cnt[3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, L = 2 * nc + 1;
  int c0 = 0, c1 = 0, c2 = 0;
  for (int n = tid; n < N; n += 1024) {
    const int a = mask_t[n], b = inst_t[n];
    c0 += (a >= 0 && a < nc); c1 += (b >= 0 && b < nc); c2 += (edge_t[n] >= 0.f);
  }
  c0 = wave_sum_int(c0); c1 = wave_sum_int(c1); c2 = wave_sum_int(c2);
  if (lane == 0) { cnt_w[0][wave] = c0; cnt_w[1][wave] = c1; cnt_w[2][wave] = c2; }
  __syncthreads();
  if (tid < 3) {
    int s = 0;
    for (int v = 0; v < 16; ++v) s += cnt_w[tid][v];
    cnt[tid] = s;
  }
  __syncthreads();
  const int n0 = cnt[0], n1 = cnt[1], n2 = cnt[2];
  const float sc[3] = {n0 > 0 ? wm / (float)n0 : 0.f, n1 > 0 ? wi / (float)n1 : 0.f, n2 > 0 ? we / (float)n2 : 0.f};
  double a[3] = {0.0, 0.0, 0.0};
  for (int n = tid; n < N; n += 1024) {
    const float* l = logits + (size_t)n * L;
    float* d = dlogits + (size_t)n * L;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = h ? inst_t[n] : mask_t[n];
      const float* lh = l + h * nc;
      float* dh = d + h * nc;
      if (t < 0 || t >= nc) {
        for (int c = 0; c < nc; ++c) dh[c] = 0.f;
      } else {
        float mx = lh[0];
        for (int c = 1; c < nc; ++c) mx = fmaxf(mx, lh[c]);
        float den = 0.f;
        for (int c = 0; c < nc; ++c) den += expf(lh[c] - mx);
        a[h] += (double)(mx + logf(den) - lh[t]);
        for (int c = 0; c < nc; ++c) dh[c] = (expf(lh[c] - mx) / den - (c == t ? 1.f : 0.f)) * sc[h];
      }
    }
    const float t = edge_t[n], z = l[2 * nc];
    if (t >= 0.f) {
      a[2] += (double)(fmaxf(z, 0.f) - z * t + logf(1.0f + expf(-fabsf(z))));
      d[2 * nc] = (1.0f / (1.0f + expf(-z)) - t) * sc[2];
    } else {
      d[2 * nc] = 0.f;
    }
  }
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const double v = wave_sum_f64(a[h]);
    if (lane == 0) sum_w[h][wave] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double term[3];
    for (int h = 0; h < 3; ++h) {
      double s = 0.0;
      for (int v = 0; v < 16; ++v) s += sum_w[h][v];
      term[h] = cnt[h] > 0 ? s / (double)cnt[h] : 0.0;
    }
    loss[0] = (float)((double)wm * term[0] + (double)wi * term[1] + (double)we * term[2]);
    loss[1] = (float)term[0]; loss[2] = (float)term[1]; loss[3] = (float)term[2];
  }
}

// ---- structure loss on the painted mask (include/camo_rg_pixel_loss.h) ----------------------------------------
// An image's five sums, each a double: SA, SB, I = sum p B, sum p A, sum [B sp(-z) + (A - B) sp(z)].
struct PixSums { double sa, sb, i, pa, w; };
struct PixNode { double A, B, p; float z; };

__device__ __forceinline__ float softplus_f32(float z) { return fmaxf(z, 0.f) + logf(1.0f + expf(-fabsf(z))); }

__device__ __forceinline__ PixNode pix_node(const float* __restrict__ logits, const long long* __restrict__ node_w, int v, int L) {
  const float* l = logits + (size_t)v * L;
  const float z = l[1] - l[0];
  return PixNode{(double)node_w[2 * (size_t)v], (double)node_w[2 * (size_t)v + 1], (double)(1.0f / (1.0f + expf(-z))), z};
}

// the caller's share of the sums of the nodes lo .. hi - 1: lo + first, lo + first + stride, ... in that order
__device__ __forceinline__ PixSums pix_partial(const float* __restrict__ logits, const long long* __restrict__ node_w, int lo, int hi, int first,
                                               int stride, int L) {
  PixSums s{0.0, 0.0, 0.0, 0.0, 0.0};
  for (int v = lo + first; v < hi; v += stride) {
    const PixNode n = pix_node(logits, node_w, v, L);
    s.sa += n.A; s.sb += n.B; s.i += n.p * n.B; s.pa += n.p * n.A;
    s.w += n.B * (double)softplus_f32(-n.z) + (n.A - n.B) * (double)softplus_f32(n.z);
  }
  return s;
}

__device__ __forceinline__ PixSums pix_wave_sum(PixSums s) {
  return PixSums{wave_sum_f64(s.sa), wave_sum_f64(s.sb), wave_sum_f64(s.i), wave_sum_f64(s.pa), wave_sum_f64(s.w)};
}

// node_off[i] clamped to [0, N]; a decreasing pair is an empty image
__device__ __forceinline__ void pix_range(const int* __restrict__ node_off, int i, int N, int& lo, int& hi) {
  lo = min(max(node_off[i], 0), N);
  hi = max(min(max(node_off[i + 1], 0), N), lo);
}

// grid n_images, block 256: ONE block per image.  n_img first (every block counts the images with SA > 0 itself, a wave per image:
// integer sums, so all blocks agree), then the image's five sums -- per-thread doubles in node order, a butterfly per wave, the 4
// waves in order -- then per node t = w_pixel dP/dz in double, rounded once, added to dlogits[v][1] and subtracted from dlogits[v][0].
__global__ __launch_bounds__(256) void rgt_pixel_loss_kernel(const float* __restrict__ logits, const long long* __restrict__ node_w,
                                                             const int* __restrict__ node_off, int n_images, int N, int L, double K,
                                                             float w_pixel, float* __restrict__ dlogits) {
  __shared__ int cnt_w[4];
  __shared__ double sum_w[5][4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int lo, hi;
  pix_range(node_off, blockIdx.x, N, lo, hi);
  if (hi == lo || !(w_pixel > 0.f)) return;
  int c = 0;
  for (int j = wave; j < n_images; j += 4) {
    int a, b;
    pix_range(node_off, j, N, a, b);
    unsigned long long s = 0;
    for (int v = a + lane; v < b; v += 64) s += (unsigned long long)node_w[2 * (size_t)v];
    c += (long long)wave_sum_u64(s) > 0;
  }
  if (lane == 0) cnt_w[wave] = c;
  const PixSums part = pix_wave_sum(pix_partial(logits, node_w, lo, hi, tid, 256, L));
  if (lane == 0) { sum_w[0][wave] = part.sa; sum_w[1][wave] = part.sb; sum_w[2][wave] = part.i; sum_w[3][wave] = part.pa; sum_w[4][wave] = part.w; }
  __syncthreads();
  double t[5];
  for (int k = 0; k < 5; ++k) t[k] = ((sum_w[k][0] + sum_w[k][1]) + sum_w[k][2]) + sum_w[k][3];
  const int n_img = cnt_w[0] + cnt_w[1] + cnt_w[2] + cnt_w[3];
  const double SA = t[0], IK = t[2] + K, D = t[3] + t[1] - t[2] + K;
  if (!(SA > 0.0) || n_img < 1) return;
  const double scale = (double)w_pixel / (double)n_img;
  for (int v = lo + tid; v < hi; v += 256) {
    const PixNode n = pix_node(logits, node_w, v, L);
    const double dz = (n.A * n.p - n.B) / SA - n.p * (1.0 - n.p) * (n.B * D - IK * (n.A - n.B)) / (D * D);
    const float g = (float)(scale * dz);
    float* d = dlogits + (size_t)v * L;
    d[1] += g;
    d[0] -= g;
  }
}

// ONE block of 1024 threads: a wave per image (the 16 waves stride over the images), its sums by one butterfly; every wave adds
// its images' wbce and wiou in image order, then the 16 waves in order.  loss[0] += w_pixel P, loss[4] = mean wbce, loss[5] = mean wiou.
__global__ __launch_bounds__(1024) void rgt_pixel_finish_kernel(const float* __restrict__ logits, const long long* __restrict__ node_w,
                                                                const int* __restrict__ node_off, int n_images, int N, int L, double K,
                                                                float w_pixel, float* __restrict__ loss) {
  __shared__ int cnt_w[16];
  __shared__ double sum_w[2][16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int c = 0;
  double bce = 0.0, iou = 0.0;
  for (int j = wave; j < n_images; j += 16) {
    int lo, hi;
    pix_range(node_off, j, N, lo, hi);
    const PixSums s = pix_wave_sum(pix_partial(logits, node_w, lo, hi, lane, 64, L));
    if (s.sa > 0.0) {
      ++c;
      bce += s.w / s.sa;
      iou += 1.0 - (s.i + K) / (s.pa + s.sb - s.i + K);
    }
  }
  if (lane == 0) { cnt_w[wave] = c; sum_w[0][wave] = bce; sum_w[1][wave] = iou; }
  __syncthreads();
  if (tid == 0) {
    int n_img = 0;
    double b = 0.0, u = 0.0;
    for (int v = 0; v < 16; ++v) { n_img += cnt_w[v]; b += sum_w[0][v]; u += sum_w[1][v]; }
    if (n_img > 0) { b /= (double)n_img; u /= (double)n_img; }
    if (w_pixel > 0.f) loss[0] = (float)((double)loss[0] + (double)w_pixel * (b + u));
    loss[4] = (float)b; loss[5] = (float)u;
  }
}

// ---- dense pieces that are too thin for the GEMM --------------------------------------------------------------------------
// scale: 1 / (1 - p_head) when Z is the dropped activation (Z > 0 then says "kept and open"), else 1
__global__ void head_dz_kernel(HeadPtrs P, const float* __restrict__ Z, const float* __restrict__ dlogits, float* __restrict__ dZ,
                               long long total, int H, int nc, float scale) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return;
  const int Hh = H >> 1, units = 3 * Hh, L = 2 * nc + 1;
  const long long n = idx / units;
  const int u = (int)(idx - n * units), h = u / Hh, j = u - h * Hh, nch = h < 2 ? nc : 1;
  float v = 0.f;
  if (Z[idx] > 0.f) {
    const float* dl = dlogits + n * L + h * nc;
    const float* W2 = P.p[4 * h + 2];
    for (int c = 0; c < nch; ++c) v = fmaf(dl[c], W2[(size_t)c * Hh + j], v);
    v *= scale;
  }
  dZ[idx] = v;
}

// grid (row blocks, column blocks): thread = output (m, c), the block's rows in increasing order
__global__ void cross_partial_kernel(const float* __restrict__ A, int lda, int MA, const float* __restrict__ B, int ldb, int NB, int N,
                                     float* __restrict__ partial) {
  const int idx = blockIdx.y * NT + threadIdx.x, W = MA * NB;
  if (idx >= W) return;
  const int mi = idx / NB, c = idx - mi * NB;
  const int r0 = blockIdx.x * RGT_ROWS, r1 = min(N, r0 + RGT_ROWS);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s = fmaf(A ? A[(size_t)r * lda + mi] : 1.0f, B[(size_t)r * ldb + c], s);
  partial[(size_t)blockIdx.x * W + idx] = s;
}

__global__ void colsum_finish_kernel(const float* __restrict__ partial, int nb, int width, RgtSegs segs) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= width) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += partial[(size_t)b * width + c];
  for (int g = 0; g < segs.n; ++g)
    if (c >= segs.beg[g] && c < segs.beg[g + 1]) segs.out[g][c - segs.beg[g]] = s;
}

// BATCH (batch statistics): the two partial sums only; d is left as it is, bn is not read (bn_dz_kernel needs the finished sums first)
template <bool BATCH>
__global__ void bn_backward_kernel(float* __restrict__ d, const float* __restrict__ xhat, BnEval bn, int N, int C, float* __restrict__ partial) {
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= C) return;
  float scale = 0.f;
  if constexpr (!BATCH) scale = bn.weight[c] / sqrtf(bn.var[c] + BN_EPS);
  const int r0 = blockIdx.x * RGT_ROWS, r1 = min(N, r0 + RGT_ROWS);
  float s0 = 0.f, s1 = 0.f;
  for (int r = r0; r < r1; ++r) {
    const size_t at = (size_t)r * C + c;
    const float dy = d[at];
    s0 = fmaf(dy, xhat[at], s0);
    s1 += dy;
    if constexpr (!BATCH) d[at] = dy * scale;
  }
  partial[((size_t)blockIdx.x * 2) * C + c] = s0;
  partial[((size_t)blockIdx.x * 2 + 1) * C + c] = s1;
}

// BATCH: the conv bias cancels against the batch mean, so its gradient is +0.0f by definition (written as that, not as rounding noise)
template <bool BATCH>
__global__ void bn_finish_kernel(const float* __restrict__ partial, int nb, BnEval bn, int C, float* __restrict__ dweight,
                                 float* __restrict__ dbias_bn, float* __restrict__ dbias_conv) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  float s0 = 0.f, s1 = 0.f;
  for (int b = 0; b < nb; ++b) { s0 += partial[((size_t)b * 2) * C + c]; s1 += partial[((size_t)b * 2 + 1) * C + c]; }
  dweight[c] = s0;
  dbias_bn[c] = s1;
  if constexpr (BATCH) dbias_conv[c] = 0.f;
  else dbias_conv[c] = s1 * (bn.weight[c] / sqrtf(bn.var[c] + BN_EPS));
}

// ---- batch statistics (include/camo_rg_train_bn.h) ---------------------------------------------------------------------------
// Column statistics of z [N, C] in two stages, thread = channel (consecutive lanes on consecutive channels), never E[z^2] - mean^2.
// Stage 1, grid (row blocks, column blocks): the block's rows in increasing order, twice -- their mean, then the centred squares
// M2 = sum (z - mean)^2 (the second walk hits the cache).  partial[b, 0 | 1, c] = mean | M2.
__global__ void bn_stats_partial_kernel(const float* __restrict__ z, int N, int C, float* __restrict__ partial) {
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= C) return;
  const int r0 = blockIdx.x * RGT_ROWS, r1 = min(N, r0 + RGT_ROWS);
  const float z0 = z[(size_t)r0 * C + c];      // the sum is taken about the block's first row: a common offset of z costs no digits
  float s = 0.f;
  for (int r = r0 + 1; r < r1; ++r) s += z[(size_t)r * C + c] - z0;
  const float mean = z0 + s / (float)(r1 - r0);
  float m2 = 0.f;
  for (int r = r0; r < r1; ++r) { const float d = z[(size_t)r * C + c] - mean; m2 = fmaf(d, d, m2); }
  partial[((size_t)blockIdx.x * 2) * C + c] = mean;
  partial[((size_t)blockIdx.x * 2 + 1) * C + c] = m2;
}

// Chan's update: (mean, m2) over na rows absorbs (mb, qb) over nbk >= 1 rows
__device__ __forceinline__ void chan_merge(float& mean, float& m2, int& na, float mb, float qb, int nbk) {
  const int n = na + nbk;
  const float delta = mb - mean;
  mean += delta * ((float)nbk / (float)n);
  m2 += qb + delta * delta * ((float)na * (float)nbk / (float)n);
  na = n;
}

// Stage 2, block = 16 channels x 16 groups: group g merges its contiguous run of ceil(nb / 16) row blocks in block order (Chan's
// update; the last block may hold fewer rows), then the thread of group 0 merges the 16 runs in group order and owns the channel: a
// fixed order at both levels, and a chain of nb / 16 + 16 dependent steps in place of nb.  It writes mean and rstd = 1 / sqrt(var +
// 1e-5) for the kernels below, (mean, biased var) for the caller, and the running update
// running <- (1 - momentum) running + momentum (mean | var N / (N - 1)).  The three optional outputs may be null.
constexpr int BN_FIN_CH = 16, BN_FIN_GROUPS = 16;
__global__ void bn_stats_finish_kernel(const float* __restrict__ partial, int nb, int N, int C, float momentum, float* __restrict__ mean_out,
                                       float* __restrict__ rstd_out, float* __restrict__ batch_stats, float* __restrict__ running_mean,
                                       float* __restrict__ running_var) {
  __shared__ float sh_mean[BN_FIN_GROUPS][BN_FIN_CH], sh_m2[BN_FIN_GROUPS][BN_FIN_CH];
  const int cl = threadIdx.x % BN_FIN_CH, g = threadIdx.x / BN_FIN_CH, c = blockIdx.x * BN_FIN_CH + cl;
  const int per = (nb + BN_FIN_GROUPS - 1) / BN_FIN_GROUPS;
  float mean = 0.f, m2 = 0.f;
  int na = 0;
  if (c < C) {
    for (int b = g * per; b < min(nb, (g + 1) * per); ++b) {
      const int nbk = min(N - b * RGT_ROWS, RGT_ROWS);
      const float mb = partial[((size_t)b * 2) * C + c], qb = partial[((size_t)b * 2 + 1) * C + c];
      if (na == 0) { mean = mb; m2 = qb; na = nbk; }
      else chan_merge(mean, m2, na, mb, qb, nbk);
    }
  }
  sh_mean[g][cl] = mean; sh_m2[g][cl] = m2;
  __syncthreads();
  if (g != 0 || c >= C) return;
  for (int h = 1; h < BN_FIN_GROUPS && h * per < nb; ++h) {
    const int rows = min(N, min(nb, (h + 1) * per) * RGT_ROWS) - h * per * RGT_ROWS;
    chan_merge(mean, m2, na, sh_mean[h][cl], sh_m2[h][cl], rows);
  }
  const float var = m2 / (float)N;
  mean_out[c] = mean;
  rstd_out[c] = 1.0f / sqrtf(var + BN_EPS);
  if (batch_stats) { batch_stats[c] = mean; batch_stats[C + c] = var; }
  if (running_mean) {
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (var * ((float)N / (float)(N - 1)));
  }
}

// The two elementwise passes: grid (blocks of BN_EW_ROWS rows, column blocks), thread = channel, which reads its channel's four
// constants once and walks the block's rows (no index division; a wave's lanes stay on consecutive channels of one row).
constexpr int BN_EW_ROWS = 16;

// in place zx = xhat = (z - mean) * rstd, out = relu(xhat * weight + bias); DROP (bn_apply_drop_kernel only): out *= the keep
// multiplier of element r * C + c
template <bool DROP>
__device__ __forceinline__ void bn_apply_body(float* __restrict__ zx, const float* __restrict__ mean, const float* __restrict__ rstd,
                                              const float* __restrict__ weight, const float* __restrict__ bias, float* __restrict__ out, int N, int C,
                                              const DropCfg& drop, uint32_t site) {
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= C) return;
  const float mu = mean[c], rs = rstd[c], g = weight[c], b = bias[c];
  const int r0 = blockIdx.x * BN_EW_ROWS, r1 = min(N, r0 + BN_EW_ROWS);
  for (int r = r0; r < r1; ++r) {
    const size_t at = (size_t)r * C + c;
    const float xh = (zx[at] - mu) * rs;
    zx[at] = xh;
    float y = fmaxf(xh * g + b, 0.f);
    if constexpr (DROP) y *= drop_mult(drop, site, (uint32_t)r * (uint32_t)C + (uint32_t)c);
    out[at] = y;
  }
}

__global__ void bn_apply_kernel(float* __restrict__ zx, const float* __restrict__ mean, const float* __restrict__ rstd,
                                const float* __restrict__ weight, const float* __restrict__ bias, float* __restrict__ out, int N, int C) {
  bn_apply_body<false>(zx, mean, rstd, weight, bias, out, N, C, DropCfg{}, 0u);
}

__global__ void bn_apply_drop_kernel(float* __restrict__ zx, const float* __restrict__ mean, const float* __restrict__ rstd,
                                     const float* __restrict__ weight, const float* __restrict__ bias, float* __restrict__ out, int N, int C,
                                     DropCfg drop, uint32_t site) {
  bn_apply_body<true>(zx, mean, rstd, weight, bias, out, N, C, drop, site);
}

// in place d = dz = weight rstd (dy - dbias / N - xhat dweight / N), dweight and dbias being the finished column sums
__global__ void bn_dz_kernel(float* __restrict__ d, const float* __restrict__ xhat, const float* __restrict__ weight,
                             const float* __restrict__ rstd, const float* __restrict__ dweight, const float* __restrict__ dbias, int N, int C,
                             float inv_n) {
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= C) return;
  const float scale = weight[c] * rstd[c], mb = dbias[c] * inv_n, mw = dweight[c] * inv_n;
  const int r0 = blockIdx.x * BN_EW_ROWS, r1 = min(N, r0 + BN_EW_ROWS);
  for (int r = r0; r < r1; ++r) {
    const size_t at = (size_t)r * C + c;
    d[at] = scale * (d[at] - mb - xhat[at] * mw);
  }
}

// ---- sparse backward ------------------------------------------------------------------------------------------------------------
// one wave per SOURCE node j, 4 nodes per block: the forward's gather over the reversed CSR, with the forward's dinv
template <int CPL>
__global__ void gcn_backward_kernel(const float* __restrict__ dPre, const int* __restrict__ rrowptr, const int* __restrict__ rcol,
                                    const float* __restrict__ rw, const float* __restrict__ dinv, float* __restrict__ dXW, int N, int C) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= N) return;
  const float dj = dinv[j];
  float acc[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) acc[q] = 0.f;
  for (int e = rrowptr[j]; e < rrowptr[j + 1]; ++e) {
    const int i = rcol[e];
    const float nrm = dj * rw[e] * dinv[i];
    const float* g = dPre + (size_t)i * C;
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < C) acc[q] = fmaf(nrm, g[c], acc[q]); }
  }
#pragma unroll
  for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; if (c < C) dXW[(size_t)j * C + c] = acc[q]; }
}

// grid N (target i), block 64 * heads.  (Every lane of a wave walks the same edges: the butterflies are wave-uniform.)
template <int CPL>
__global__ void gat_backward_a_kernel(const float* __restrict__ dPre, const float* __restrict__ Hh, const float* __restrict__ O,
                                      const float* __restrict__ a_src, const float* __restrict__ a_dst, const float* __restrict__ m,
                                      const float* __restrict__ S, const int* __restrict__ rowptr, const int* __restrict__ col,
                                      float* __restrict__ r_out, float* __restrict__ da_dst, int heads, int C) {
  const int i = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float invh = 1.0f / (float)heads;
  float g[CPL], dot = 0.f;
  const float* o = O + ((size_t)i * heads + k) * C;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = lane + 64 * q;
    g[q] = c < C ? dPre[(size_t)i * C + c] * invh : 0.f;
    dot = fmaf(g[q], c < C ? o[c] : 0.f, dot);
  }
  const float r = wave_sum(dot);
  const float ad = a_dst[i * heads + k], mm = m[i * heads + k], den = S[i * heads + k];
  float dd = 0.f;
  for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
    const int j = col[e];
    const float s = a_src[j * heads + k] + ad;
    const float alpha = expf(lrelu(s) - mm) / den;
    const float* h = Hh + ((size_t)j * heads + k) * C;
    float da = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; da = fmaf(g[q], c < C ? h[c] : 0.f, da); }
    da = wave_sum(da);
    dd += alpha * (da - r) * (s > 0.f ? 1.0f : 0.2f);
  }
  if (lane == 0) { r_out[i * heads + k] = r; da_dst[i * heads + k] = dd; }
}

// grid N (source j), block 64 * heads
template <int CPL>
__global__ void gat_backward_b_kernel(const float* __restrict__ dPre, const float* __restrict__ Hh, const float* __restrict__ a_src,
                                      const float* __restrict__ a_dst, const float* __restrict__ m, const float* __restrict__ S,
                                      const float* __restrict__ r, const float* __restrict__ da_dst, const float* __restrict__ att_src,
                                      const float* __restrict__ att_dst, const int* __restrict__ rrowptr, const int* __restrict__ rcol,
                                      float* __restrict__ da_src, float* __restrict__ dh, int heads, int C) {
  const int j = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float invh = 1.0f / (float)heads;
  const float* h = Hh + ((size_t)j * heads + k) * C;
  float hj[CPL], acc[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) { const int c = lane + 64 * q; hj[q] = c < C ? h[c] : 0.f; acc[q] = 0.f; }
  const float as = a_src[j * heads + k];
  float dsum = 0.f;
  for (int e = rrowptr[j]; e < rrowptr[j + 1]; ++e) {
    const int i = rcol[e];
    const float s = as + a_dst[i * heads + k];
    const float alpha = expf(lrelu(s) - m[i * heads + k]) / S[i * heads + k];
    float g[CPL], da = 0.f;
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      const int c = lane + 64 * q;
      g[q] = c < C ? dPre[(size_t)i * C + c] * invh : 0.f;
      da = fmaf(g[q], hj[q], da);
    }
    da = wave_sum(da);
    dsum += alpha * (da - r[i * heads + k]) * (s > 0.f ? 1.0f : 0.2f);
#pragma unroll
    for (int q = 0; q < CPL; ++q) acc[q] = fmaf(alpha, g[q], acc[q]);
  }
  const float dd = da_dst[j * heads + k];
  float* out = dh + ((size_t)j * heads + k) * C;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int c = lane + 64 * q;
    if (c < C) out[c] = acc[q] + dsum * att_src[k * C + c] + dd * att_dst[k * C + c];
  }
  if (lane == 0) da_src[j * heads + k] = dsum;
}

__global__ void att_partial_kernel(const float* __restrict__ da_src, const float* __restrict__ da_dst, const float* __restrict__ Hh, int N,
                                   int heads, int C, float* __restrict__ partial) {
  const int idx = blockIdx.y * NT + threadIdx.x, KC = heads * C;
  if (idx >= KC) return;
  const int k = idx / C;
  const int r0 = blockIdx.x * RGT_ROWS, r1 = min(N, r0 + RGT_ROWS);
  float s0 = 0.f, s1 = 0.f;
  for (int n = r0; n < r1; ++n) {
    const float h = Hh[(size_t)n * KC + idx];
    s0 = fmaf(da_src[n * heads + k], h, s0);
    s1 = fmaf(da_dst[n * heads + k], h, s1);
  }
  partial[((size_t)blockIdx.x * 2) * KC + idx] = s0;
  partial[((size_t)blockIdx.x * 2 + 1) * KC + idx] = s1;
}

HeadPtrs head_ptrs(const float* const* hp) {
  HeadPtrs P;
  for (int i = 0; i < 12; ++i) P.p[i] = hp[i];
  return P;
}

}  // namespace

int launch_rgt_gat_forward(const float* Hh, const float* a_src, const float* a_dst, const int* rowptr, const int* col, const float* bias,
                           BnEval bn, float* m, float* S, float* O, float* xhat, float* out, int N, int heads, int C, hipStream_t stream,
                           bool raw, const DropCfg* drop, uint32_t site) {
  if (heads < 1 || heads > 8 || C > 512 || (drop && raw)) return (int)hipErrorInvalidValue;
  if (drop) {
    if (C <= 128) hipLaunchKernelGGL(gat_forward_drop_kernel<2>, dim3(N), dim3(64 * heads), 0, stream, Hh, a_src, a_dst, rowptr, col, bias, bn, m, S, O, xhat, out, heads, C, *drop, site);
    else          hipLaunchKernelGGL(gat_forward_drop_kernel<8>, dim3(N), dim3(64 * heads), 0, stream, Hh, a_src, a_dst, rowptr, col, bias, bn, m, S, O, xhat, out, heads, C, *drop, site);
    return (int)hipGetLastError();
  }
  if (raw) {
    if (C <= 128) hipLaunchKernelGGL((gat_forward_kernel<2, true>), dim3(N), dim3(64 * heads), 0, stream, Hh, a_src, a_dst, rowptr, col, bias, bn, m, S, O, xhat, out, heads, C);
    else          hipLaunchKernelGGL((gat_forward_kernel<8, true>), dim3(N), dim3(64 * heads), 0, stream, Hh, a_src, a_dst, rowptr, col, bias, bn, m, S, O, xhat, out, heads, C);
    return (int)hipGetLastError();
  }
  if (C <= 128) hipLaunchKernelGGL(gat_forward_kernel<2>, dim3(N), dim3(64 * heads), 0, stream, Hh, a_src, a_dst, rowptr, col, bias, bn, m, S, O, xhat, out, heads, C);
  else          hipLaunchKernelGGL(gat_forward_kernel<8>, dim3(N), dim3(64 * heads), 0, stream, Hh, a_src, a_dst, rowptr, col, bias, bn, m, S, O, xhat, out, heads, C);
  return (int)hipGetLastError();
}

int launch_rgt_concat_heads(const float* const* hp, float* W1, float* b1, int hidden, hipStream_t stream) {
  const int total = 3 * (hidden / 2) * (hidden + 1);
  hipLaunchKernelGGL(concat_heads_kernel, dim3((total + NT - 1) / NT), dim3(NT), 0, stream, head_ptrs(hp), W1, b1, hidden);
  return (int)hipGetLastError();
}

int launch_rgt_head_logits(const float* const* hp, const float* Z, float* logits, int N, int hidden, int nc, hipStream_t stream) {
  hipLaunchKernelGGL(head_logits_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, head_ptrs(hp), Z, logits, N, hidden, nc);
  return (int)hipGetLastError();
}

int launch_rgt_loss(const float* logits, const int* mask_t, const int* inst_t, const float* edge_t, float wm, float wi, float we, int N,
                    int nc, float* loss, float* dlogits, hipStream_t stream) {
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(1024), 0, stream, logits, mask_t, inst_t, edge_t, wm, wi, we, N, nc, loss, dlogits);
  return (int)hipGetLastError();
}

int launch_rgt_pixel_loss(const float* logits, const RgPixel& px, int N, int nc, float* loss, float* dlogits, hipStream_t stream) {
  const int L = 2 * nc + 1, win = 2 * px.radius + 1;
  const double K = (double)(win * win);
  hipLaunchKernelGGL(rgt_pixel_loss_kernel, dim3((unsigned)px.n_images), dim3(256), 0, stream, logits, px.node_w, px.node_off, px.n_images, N, L,
                     K, px.w_pixel, dlogits);
  hipLaunchKernelGGL(rgt_pixel_finish_kernel, dim3(1), dim3(1024), 0, stream, logits, px.node_w, px.node_off, px.n_images, N, L, K, px.w_pixel,
                     loss);
  return (int)hipGetLastError();
}

int launch_rgt_head_dz(const float* const* hp, const float* Z, const float* dlogits, float* dZ, int N, int hidden, int nc, hipStream_t stream,
                       float scale) {
  const long long total = (long long)N * 3 * (hidden / 2);
  hipLaunchKernelGGL(head_dz_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, head_ptrs(hp), Z, dlogits, dZ, total, hidden, nc, scale);
  return (int)hipGetLastError();
}

int launch_rgt_cross_partial(const float* A, int lda, int MA, const float* B, int ldb, int NB, int N, float* partial, hipStream_t stream) {
  hipLaunchKernelGGL(cross_partial_kernel, dim3(rgt_row_blocks(N), (MA * NB + NT - 1) / NT), dim3(NT), 0, stream, A, lda, MA, B, ldb, NB, N, partial);
  return (int)hipGetLastError();
}

int launch_rgt_colsum_finish(const float* partial, int nb, int width, RgtSegs segs, hipStream_t stream) {
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((width + NT - 1) / NT), dim3(NT), 0, stream, partial, nb, width, segs);
  return (int)hipGetLastError();
}

int launch_rgt_bn_backward(float* d, const float* xhat, BnEval bn, int N, int C, float* partial, hipStream_t stream, bool batch) {
  const dim3 grid(rgt_row_blocks(N), (C + NT - 1) / NT);
  if (batch) hipLaunchKernelGGL(bn_backward_kernel<true>, grid, dim3(NT), 0, stream, d, xhat, bn, N, C, partial);
  else       hipLaunchKernelGGL(bn_backward_kernel<false>, grid, dim3(NT), 0, stream, d, xhat, bn, N, C, partial);
  return (int)hipGetLastError();
}

int launch_rgt_bn_finish(const float* partial, int nb, BnEval bn, int C, float* dweight, float* dbias_bn, float* dbias_conv, hipStream_t stream,
                         bool batch) {
  const dim3 grid((C + NT - 1) / NT);
  if (batch) hipLaunchKernelGGL(bn_finish_kernel<true>, grid, dim3(NT), 0, stream, partial, nb, bn, C, dweight, dbias_bn, dbias_conv);
  else       hipLaunchKernelGGL(bn_finish_kernel<false>, grid, dim3(NT), 0, stream, partial, nb, bn, C, dweight, dbias_bn, dbias_conv);
  return (int)hipGetLastError();
}

int launch_rgt_bn_stats(const float* z, int N, int C, float momentum, float* partial, float* mean, float* rstd, float* batch_stats,
                        float* running_mean, float* running_var, hipStream_t stream) {
  if (N < 2) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(rgt_row_blocks(N), (C + NT - 1) / NT), dim3(NT), 0, stream, z, N, C, partial);
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + BN_FIN_CH - 1) / BN_FIN_CH), dim3(BN_FIN_CH * BN_FIN_GROUPS), 0, stream, partial,
                     rgt_row_blocks(N), N, C, momentum, mean, rstd, batch_stats, running_mean, running_var);
  return (int)hipGetLastError();
}

int launch_rgt_bn_apply(float* zx, const float* mean, const float* rstd, const float* weight, const float* bias, float* out, int N, int C,
                        hipStream_t stream, const DropCfg* drop, uint32_t site) {
  const dim3 grid((N + BN_EW_ROWS - 1) / BN_EW_ROWS, (C + NT - 1) / NT);
  if (drop) hipLaunchKernelGGL(bn_apply_drop_kernel, grid, dim3(NT), 0, stream, zx, mean, rstd, weight, bias, out, N, C, *drop, site);
  else      hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(NT), 0, stream, zx, mean, rstd, weight, bias, out, N, C);
  return (int)hipGetLastError();
}

int launch_rgt_bn_dz(float* d, const float* xhat, const float* weight, const float* rstd, const float* dweight, const float* dbias, int N, int C,
                     hipStream_t stream) {
  hipLaunchKernelGGL(bn_dz_kernel, dim3((N + BN_EW_ROWS - 1) / BN_EW_ROWS, (C + NT - 1) / NT), dim3(NT), 0, stream, d, xhat, weight, rstd, dweight,
                     dbias, N, C, 1.0f / (float)N);
  return (int)hipGetLastError();
}

int launch_rgt_gcn_backward(const float* dPre, const int* rrowptr, const int* rcol, const float* rw, const float* dinv, float* dXW, int N,
                            int C, hipStream_t stream) {
  if (C > 512) return (int)hipErrorInvalidValue;
  if (C <= 128) hipLaunchKernelGGL(gcn_backward_kernel<2>, dim3((N + 3) / 4), dim3(256), 0, stream, dPre, rrowptr, rcol, rw, dinv, dXW, N, C);
  else          hipLaunchKernelGGL(gcn_backward_kernel<8>, dim3((N + 3) / 4), dim3(256), 0, stream, dPre, rrowptr, rcol, rw, dinv, dXW, N, C);
  return (int)hipGetLastError();
}

int launch_rgt_gat_backward_a(const float* dPre, const float* Hh, const float* O, const float* a_src, const float* a_dst, const float* m,
                              const float* S, const int* rowptr, const int* col, float* r, float* da_dst, int N, int heads, int C,
                              hipStream_t stream) {
  if (heads < 1 || heads > 8 || C > 512) return (int)hipErrorInvalidValue;
  if (C <= 128) hipLaunchKernelGGL(gat_backward_a_kernel<2>, dim3(N), dim3(64 * heads), 0, stream, dPre, Hh, O, a_src, a_dst, m, S, rowptr, col, r, da_dst, heads, C);
  else          hipLaunchKernelGGL(gat_backward_a_kernel<8>, dim3(N), dim3(64 * heads), 0, stream, dPre, Hh, O, a_src, a_dst, m, S, rowptr, col, r, da_dst, heads, C);
  return (int)hipGetLastError();
}

int launch_rgt_gat_backward_b(const float* dPre, const float* Hh, const float* a_src, const float* a_dst, const float* m, const float* S,
                              const float* r, const float* da_dst, const float* att_src, const float* att_dst, const int* rrowptr,
                              const int* rcol, float* da_src, float* dh, int N, int heads, int C, hipStream_t stream) {
  if (heads < 1 || heads > 8 || C > 512) return (int)hipErrorInvalidValue;
  if (C <= 128) hipLaunchKernelGGL(gat_backward_b_kernel<2>, dim3(N), dim3(64 * heads), 0, stream, dPre, Hh, a_src, a_dst, m, S, r, da_dst, att_src, att_dst, rrowptr, rcol, da_src, dh, heads, C);
  else          hipLaunchKernelGGL(gat_backward_b_kernel<8>, dim3(N), dim3(64 * heads), 0, stream, dPre, Hh, a_src, a_dst, m, S, r, da_dst, att_src, att_dst, rrowptr, rcol, da_src, dh, heads, C);
  return (int)hipGetLastError();
}

int launch_rgt_att_partial(const float* da_src, const float* da_dst, const float* Hh, int N, int heads, int C, float* partial,
                           hipStream_t stream) {
  hipLaunchKernelGGL(att_partial_kernel, dim3(rgt_row_blocks(N), (heads * C + NT - 1) / NT), dim3(NT), 0, stream, da_src, da_dst, Hh, N, heads, C, partial);
  return (int)hipGetLastError();
}
