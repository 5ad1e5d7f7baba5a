// Region-graph detector (include/camo_rg_detect.h): what turns node embeddings into a pixel mask and its score.
// ~25 k multiply-adds per node, one gather per pixel and five sums per image: the cost is launches, so each step is ONE launch
// over the whole batch (the counts take a clear before them).
#include "rg_detect.h"

#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int KC = 32;            // input features per staged chunk
constexpr int WS = KC + 1;        // row stride of the weight chunk in LDS: odd, so the 64 rows a wave reads lie in 64 banks
constexpr int LG = 17;            // row stride of a tile's logits in LDS: 2 * 8 + 1

// Block = T node rows.  First layers: thread t owns hidden unit u0 + t of the 3 * hidden / 2 units of the three heads (mask |
// instance | edge) for all T rows; the units' weight rows and the rows' embeddings come through LDS in chunks of KC inputs --
// global reads of 128 contiguous bytes per row, LDS reads of one bank per lane (weights) or one address per wave (embeddings).
// Second layers: one wave per (row, logit), lanes over the hidden units, a butterfly sum.  Then one thread per row: probabilities.
// Dynamic LDS: w [NT][WS] | e [T][KC] | lg [T][LG] | z [T][3 * hidden / 2]   (under 64 KB for both instantiations)
template <int T>
__global__ __launch_bounds__(NT) void rgd_heads_kernel(RgdHeads P, const float* __restrict__ emb, int n, int H, int nc,
                                                       float* __restrict__ logits, float* __restrict__ probs) {
  extern __shared__ float lds[];
  float* w_tile = lds;
  float* e_tile = w_tile + NT * WS;          // (byte offset 33792: 16-byte aligned for the float4 reads)
  float* lg = e_tile + T * KC;
  float* z = lg + T * LG;
  const int Hh = H >> 1, units = 3 * Hh, L = 2 * nc + 1;
  const int tid = threadIdx.x, row0 = blockIdx.x * T;
  const int lc = tid & (KC - 1), lr = tid / KC;

  for (int u0 = 0; u0 < units; u0 += NT) {
    float acc[T];
#pragma unroll
    for (int r = 0; r < T; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += KC) {
      __syncthreads();                                              // the chunk before this one has been read
      const int k = k0 + lc;
      for (int i = 0; i < KC; ++i) {                                // NT / KC = 8 rows per pass, 32 passes: NT rows
        const int r = lr + (NT / KC) * i, u = u0 + r;
        float v = 0.f;
        if (u < units && k < H) {
          const int h = (u >= Hh) + (u >= 2 * Hh);
          const float* W1 = h == 0 ? P.p[0] : h == 1 ? P.p[4] : P.p[8];
          v = W1[(size_t)(u - h * Hh) * H + k];
        }
        w_tile[r * WS + lc] = v;
      }
      for (int idx = tid; idx < T * KC; idx += NT) {
        const int row = row0 + idx / KC;
        e_tile[idx] = (row < n && k < H) ? emb[(size_t)row * H + k] : 0.f;      // (idx % KC == lc: NT is a multiple of KC)
      }
      __syncthreads();
      const float* wr = w_tile + tid * WS;
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        const float w0 = wr[kk], w1 = wr[kk + 1], w2 = wr[kk + 2], w3 = wr[kk + 3];
#pragma unroll
        for (int r = 0; r < T; ++r) {
          const float4 e = *reinterpret_cast<const float4*>(e_tile + r * KC + kk);
          acc[r] = fmaf(w3, e.w, fmaf(w2, e.z, fmaf(w1, e.y, fmaf(w0, e.x, acc[r]))));
        }
      }
    }
    const int u = u0 + tid;
    if (u < units) {
      const int h = (u >= Hh) + (u >= 2 * Hh);
      const float* B1 = h == 0 ? P.p[1] : h == 1 ? P.p[5] : P.p[9];
      const float b = B1[u - h * Hh];
#pragma unroll
      for (int r = 0; r < T; ++r) z[r * units + u] = fmaxf(acc[r] + b, 0.f);
    }
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  for (int idx = wave; idx < T * L; idx += NT / 64) {
    const int r = idx / L, o = idx - r * L;
    const int h = (o >= nc) + (o >= 2 * nc), c = o - h * nc;
    const float* W2 = (h == 0 ? P.p[2] : h == 1 ? P.p[6] : P.p[10]) + (size_t)c * Hh;
    const float* B2 = h == 0 ? P.p[3] : h == 1 ? P.p[7] : P.p[11];
    const float* zr = z + r * units + h * Hh;
    float s = 0.f;
    for (int j = lane; j < Hh; j += 64) s = fmaf(W2[j], zr[j], s);
    s = wave_sum(s);
    if (lane == 0) {
      const float v = s + B2[c];
      lg[r * LG + o] = v;
      if (row0 + r < n) logits[(size_t)(row0 + r) * L + o] = v;
    }
  }
  __syncthreads();

  if (tid < T && row0 + tid < n) {
    const float* l = lg + tid * LG;
    float p[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* lh = l + h * nc;
      float m = lh[0];
      for (int c = 1; c < nc; ++c) m = fmaxf(m, lh[c]);
      float den = 0.f;
      for (int c = 0; c < nc; ++c) den += __expf(lh[c] - m);
      p[h] = __expf(lh[1] - m) / den;
    }
    float* out = probs + (size_t)(row0 + tid) * 3;
    out[0] = p[0]; out[1] = p[1]; out[2] = 1.0f / (1.0f + __expf(-l[2 * nc]));
  }
}

template <int T>
size_t heads_lds_bytes(int hidden) { return (size_t)(NT * WS + T * KC + T * LG + T * 3 * (hidden / 2)) * sizeof(float); }

// one thread per pixel of the batch; a channel's plane is written by consecutive lanes
__global__ __launch_bounds__(NT) void rgd_paint_kernel(const float* __restrict__ values, int n_nodes, int C, const int* __restrict__ seg,
                                                       const int* __restrict__ rmap, const int* __restrict__ node_off, int HW,
                                                       int label_bound, float fill, float* __restrict__ maps, long long total) {
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  const int i = (int)(p / HW), q = (int)(p - (long long)i * HW);
  const int s = seg[p];
  long long row = -1;
  if (s >= 0 && s < label_bound) {
    const int r = rmap[(size_t)i * label_bound + s];
    if (r >= 0) {
      row = (long long)node_off[i] + r;
      if (row < 0 || row >= n_nodes) row = -1;
    }
  }
  float* out = maps + (size_t)i * C * HW + q;
  for (int c = 0; c < C; ++c) out[(size_t)c * HW] = row >= 0 ? values[row * C + c] : fill;
}

__global__ void rgd_clear_kernel(unsigned long long* __restrict__ counts, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) counts[i] = 0ull;
}

// grid (blocks per image, N): a block strides over its image's pixels; per-thread integers -> wave -> block (LDS) -> five 64-bit
// integer atomics per block.  Integer addition in any order gives the same sum.
__global__ __launch_bounds__(NT) void rgd_counts_kernel(const float* __restrict__ pred, long long stride, const unsigned char* __restrict__ gt,
                                                        float threshold, int HW, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long blk[5];
  const int i = blockIdx.y, tid = threadIdx.x;
  const float* p = pred + (size_t)i * stride;
  const unsigned char* g = gt + (size_t)i * HW;
  if (tid < 5) blk[tid] = 0ull;
  __syncthreads();
  unsigned tp = 0, fp = 0, fn = 0, tn = 0;
  unsigned long long a = 0;
  for (long long q = (long long)blockIdx.x * NT + tid; q < HW; q += (long long)gridDim.x * NT) {
    const float v = p[q];
    const bool gp = g[q] > 127, pp = v > threshold;
    tp += pp && gp; fp += pp && !gp; fn += !pp && gp; tn += !pp && !gp;
    a += (unsigned long long)llrint(fabs((double)v - (gp ? 1.0 : 0.0)) * 4294967296.0);
  }
  tp = wave_sum_u32(tp); fp = wave_sum_u32(fp); fn = wave_sum_u32(fn); tn = wave_sum_u32(tn); a = wave_sum_u64(a);
  if ((tid & 63) == 0) {
    atomicAdd(&blk[0], (unsigned long long)tp); atomicAdd(&blk[1], (unsigned long long)fp); atomicAdd(&blk[2], (unsigned long long)fn);
    atomicAdd(&blk[3], (unsigned long long)tn); atomicAdd(&blk[4], a);
  }
  __syncthreads();
  if (tid < 5 && blk[tid]) atomicAdd(counts + (size_t)i * 5 + tid, blk[tid]);
}

}  // namespace

int launch_rgd_heads(const RgdHeads& P, const float* emb, int n, int hidden, int nc, float* logits, float* probs, hipStream_t stream) {
  if (hidden <= RGD_WIDE_ABOVE)
    hipLaunchKernelGGL(rgd_heads_kernel<RGD_ROWS>, dim3((n + RGD_ROWS - 1) / RGD_ROWS), dim3(NT), heads_lds_bytes<RGD_ROWS>(hidden), stream,
                       P, emb, n, hidden, nc, logits, probs);
  else
    hipLaunchKernelGGL(rgd_heads_kernel<RGD_ROWS_WIDE>, dim3((n + RGD_ROWS_WIDE - 1) / RGD_ROWS_WIDE), dim3(NT),
                       heads_lds_bytes<RGD_ROWS_WIDE>(hidden), stream, P, emb, n, hidden, nc, logits, probs);
  return (int)hipGetLastError();
}

int launch_rgd_paint(const float* values, int n_nodes, int C, const int* segments, const int* region_map, const int* node_off, int N, int H,
                     int W, int label_bound, float fill, float* maps, hipStream_t stream) {
  const long long total = (long long)N * H * W;
  hipLaunchKernelGGL(rgd_paint_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, values, n_nodes, C, segments, region_map,
                     node_off, H * W, label_bound, fill, maps, total);
  return (int)hipGetLastError();
}

int launch_rgd_counts(const float* pred, long long stride, const unsigned char* gt, float threshold, int N, int H, int W,
                      unsigned long long* counts, hipStream_t stream) {
  const int HW = H * W;
  const int per_image = std::min(std::max((HW + NT * 8 - 1) / (NT * 8), 1), 256);
  hipLaunchKernelGGL(rgd_clear_kernel, dim3((5 * N + NT - 1) / NT), dim3(NT), 0, stream, counts, 5 * N);
  hipLaunchKernelGGL(rgd_counts_kernel, dim3(per_image, N), dim3(NT), 0, stream, pred, stride, gt, threshold, HW, counts);
  return (int)hipGetLastError();
}
