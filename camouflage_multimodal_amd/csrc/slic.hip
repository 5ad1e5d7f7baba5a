// SLIC superpixel label maps of a batch of images: skimage.segmentation.slic(img_u8, n_segments, compactness, sigma) as the
// reference calls it (models/region_graph/extract_rg_embeddings.py:143-144), restated in include/camo_slic.h.  The work is
// launches and latency, as for canny.hip: every grid covers the whole batch and the launch count does not depend on N.
//
//   preprocess   one block per 32 x 32 tile, channel by channel: quantised values with a halo of the blur radius in LDS
//                (scipy's reflect boundary), Gaussian along x then y in LDS, then Lab of the three smoothed channels
//   init         centroids on the grid with zero colour; sums cleared
//   assign       one block per tile, by gather: the centroids are read 256 at a time, those whose window meets the tile are
//                compacted into LDS in ascending k (ballot prefix), and every pixel walks that list with a strict <, which
//                is the lowest-k tie rule without an atomic
//   accumulate   one block per tile: integer sums per label in a small LDS hash table (a tile meets few labels), then one
//                64-bit integer atomic per table entry and quantity to global memory; a full table falls through to
//                global atomics directly.  Integer sums: any order gives the same bits
//   finalize     one lane per centroid: divides, and leaves the sums cleared for the next round
//   connect      the 4-connected components of equal labels by cc_inl.h's tiled union-find (label tiles, join tiles; root =
//                smallest index = the component's first pixel); flatten + component sizes; one lane per small component runs its
//                breadth-first search with a queue carved from workspace, and each block counts the large components that
//                start in its chunk; exclusive prefix of the chunk counts per image; ranks of the large components; emit,
//                which follows the adopted labels of small components down to a large one or to none
//
// A small component adopts from a component with a smaller root, so the chains that emit follows end.  The queue offsets come
// from an atomic counter and differ from run to run; nothing read back depends on them.
#include <hip/hip_runtime.h>
#include "abi_util.h"
#include "cc_inl.h"
#include "label_inl.h"
#include "slic.h"

// include/camo_slic.h fixes the operation order of steps 5 and 6; hipcc contracts a * b + c by default
#pragma clang fp contract(off)

namespace {

constexpr int T = SLIC_TILE, NT = 256, PPT = T * T / NT;   // pixels per thread of a tile
constexpr int SLOTS = 128;                                 // LDS hash table of the accumulate kernel
constexpr float FIX = 16777216.0f;                         // 2^24

// scipy.ndimage mode="reflect": d c b a | a b c d | d c b a, for any distance from the image
__device__ __forceinline__ int reflect_index(int i, int n) {
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}

__device__ __forceinline__ float srgb_to_linear(float v) { return v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f; }
__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; }

__global__ __launch_bounds__(NT) void slic_preprocess_kernel(const float* __restrict__ images, int H, int W, CannyTaps taps,
                                                             float inv_compactness, float* __restrict__ lab) {
  extern __shared__ float lds[];
  const int R = taps.radius, S = T + 2 * R;
  float* v = lds;                     // [S][S] one quantised channel, rows y0 - R .., columns x0 - R ..
  float* rowb = v + S * S;            // [S][T] blurred along x
  float* sm = rowb + S * T;           // [3][T][T] smoothed channels
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const float* img = images + (size_t)n * H * W * 3;
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < S * S; i += NT) {
      const int ly = i / S, lx = i - ly * S;
      const int y = reflect_index(y0 - R + ly, H), x = reflect_index(x0 - R + lx, W);
      const float q = fminf(fmaxf(truncf(img[((size_t)y * W + x) * 3 + c] * 255.0f), 0.f), 255.f);
      v[i] = q / 255.0f;
    }
    __syncthreads();
    for (int i = tid; i < S * T; i += NT) {
      const int ly = i / T, tx = i - ly * T;
      const float* src = v + ly * S + tx;
      float s = 0.f;
      for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * src[k];
      rowb[i] = s;
    }
    __syncthreads();
    for (int i = tid; i < T * T; i += NT) {
      const int ty = i / T, tx = i - ty * T;
      const float* src = rowb + ty * T + tx;
      float s = 0.f;
      for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * src[k * T];
      sm[c * T * T + i] = s;
    }
    __syncthreads();
  }
  for (int i = tid; i < T * T; i += NT) {
    const int y = y0 + i / T, x = x0 + i % T;
    if (y >= H || x >= W) continue;
    const float r = srgb_to_linear(sm[i]), g = srgb_to_linear(sm[T * T + i]), b = srgb_to_linear(sm[2 * T * T + i]);
    const float X = ((r * 0.412453f + g * 0.357580f) + b * 0.180423f) / 0.95047f;
    const float Y = (r * 0.212671f + g * 0.715160f) + b * 0.072169f;
    const float Z = ((r * 0.019334f + g * 0.119193f) + b * 0.950227f) / 1.08883f;
    const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
    float* o = lab + ((size_t)n * H * W + (size_t)y * W + x) * 3;
    o[0] = (116.0f * fy - 16.0f) * inv_compactness;
    o[1] = (500.0f * (fx - fy)) * inv_compactness;
    o[2] = (200.0f * (fy - fz)) * inv_compactness;
  }
}

__global__ __launch_bounds__(NT) void slic_init_kernel(SlicGrid g, int N, float* __restrict__ cent, long long* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= (long long)N * g.K) return;
  const int k = (int)(i % g.K), iy = k / g.nx, ix = k - iy * g.nx;
  float* c = cent + i * 5;
  c[0] = (float)(g.start + iy * g.step); c[1] = (float)(g.start + ix * g.step);
  c[2] = 0.f; c[3] = 0.f; c[4] = 0.f;
  for (int j = 0; j < 6; ++j) sums[i * 6 + j] = 0;
}

__global__ __launch_bounds__(NT) void slic_clear_kernel(long long* __restrict__ sums, long long count) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i < count) sums[i] = 0;
}

__global__ __launch_bounds__(NT) void slic_assign_kernel(const float* __restrict__ lab, const float* __restrict__ cent, int H, int W, int K,
                                                         int step, int* __restrict__ nearest, float* __restrict__ dist) {
  __shared__ float c5[NT][5];         // the centroids of this round whose window meets the tile, in ascending k
  __shared__ int win[NT][5];          // their windows y0, y1, x0, x1 (half open) and k
  __shared__ int wcount[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.z, ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const size_t HW = (size_t)H * W;
  const float two = (float)(2 * step), w = 1.0f / (float)(step * step), fH = (float)H, fW = (float)W;
  float pl[PPT], pa[PPT], pb[PPT], best[PPT];
  int bk[PPT];
  for (int j = 0; j < PPT; ++j) {
    const int l = tid + j * NT, y = ty0 + l / T, x = tx0 + l % T;
    best[j] = INFINITY; bk[j] = 0; pl[j] = pa[j] = pb[j] = 0.f;
    if (y < H && x < W) {
      const float* p = lab + (n * HW + (size_t)y * W + x) * 3;
      pl[j] = p[0]; pa[j] = p[1]; pb[j] = p[2];
    }
  }
  for (int k0 = 0; k0 < K; k0 += NT) {
    const int k = k0 + tid;
    bool hit = false;
    float c[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int wy0 = 0, wy1 = 0, wx0 = 0, wx1 = 0;
    if (k < K) {
      const float* p = cent + ((size_t)n * K + k) * 5;
      for (int j = 0; j < 5; ++j) c[j] = p[j];
      wy0 = (int)fmaxf(c[0] - two, 0.f); wy1 = (int)fminf((c[0] + two) + 1.0f, fH);
      wx0 = (int)fmaxf(c[1] - two, 0.f); wx1 = (int)fminf((c[1] + two) + 1.0f, fW);
      hit = wy0 < ty0 + T && wy1 > ty0 && wx0 < tx0 + T && wx1 > tx0;
    }
    int total;
    const int slot = block_rank<NT>(hit, wcount, total);
    if (hit) {
      for (int j = 0; j < 5; ++j) c5[slot][j] = c[j];
      win[slot][0] = wy0; win[slot][1] = wy1; win[slot][2] = wx0; win[slot][3] = wx1; win[slot][4] = k;
    }
    __syncthreads();
    for (int j = 0; j < PPT; ++j) {
      const int l = tid + j * NT, y = ty0 + l / T, x = tx0 + l % T;
      const float fy = (float)y, fx = (float)x;
      for (int i = 0; i < total; ++i) {
        if (y < win[i][0] || y >= win[i][1] || x < win[i][2] || x >= win[i][3]) continue;
        const float ey = c5[i][0] - fy, ex = c5[i][1] - fx, el = c5[i][2] - pl[j], ea = c5[i][3] - pa[j], eb = c5[i][4] - pb[j];
        const float dy = ey * ey, dx = ex * ex;
        const float d = (dy + dx) * w + ((el * el + ea * ea) + eb * eb);
        if (d < best[j]) { best[j] = d; bk[j] = win[i][4]; }
      }
    }
    __syncthreads();
  }
  for (int j = 0; j < PPT; ++j) {
    const int l = tid + j * NT, y = ty0 + l / T, x = tx0 + l % T;
    if (y >= H || x >= W) continue;
    const size_t p = n * HW + (size_t)y * W + x;
    nearest[p] = bk[j];
    if (dist) dist[p] = best[j];
  }
}

__global__ __launch_bounds__(NT) void slic_accumulate_kernel(const float* __restrict__ lab, const int* __restrict__ nearest, int H, int W, int K,
                                                             unsigned long long* __restrict__ sums) {
  __shared__ int keys[SLOTS];
  __shared__ unsigned long long acc[SLOTS][6];
  const int tid = threadIdx.x, n = blockIdx.z, ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const size_t HW = (size_t)H * W;
  for (int i = tid; i < SLOTS; i += NT) keys[i] = -1;
  for (int i = tid; i < SLOTS * 6; i += NT) acc[i / 6][i % 6] = 0;
  __syncthreads();
  for (int j = 0; j < PPT; ++j) {
    const int l = tid + j * NT, y = ty0 + l / T, x = tx0 + l % T;
    if (y >= H || x >= W) continue;
    const size_t p = n * HW + (size_t)y * W + x;
    const int k = nearest[p];
    if ((unsigned)k >= (unsigned)K) continue;
    const float* c = lab + p * 3;
    const long long val[6] = {y, x, llrintf(c[0] * FIX), llrintf(c[1] * FIX), llrintf(c[2] * FIX), 1};
    const int slot = label_slot<SLOTS>(keys, k);
    if (slot >= 0)
      for (int q = 0; q < 6; ++q) atomicAdd(&acc[slot][q], (unsigned long long)val[q]);
    else
      for (int q = 0; q < 6; ++q) atomicAdd(sums + ((size_t)n * K + k) * 6 + q, (unsigned long long)val[q]);
  }
  __syncthreads();
  for (int i = tid; i < SLOTS * 6; i += NT) {
    const int k = keys[i / 6];
    if (k >= 0) atomicAdd(sums + ((size_t)n * K + k) * 6 + i % 6, acc[i / 6][i % 6]);
  }
}

__global__ __launch_bounds__(NT) void slic_finalize_kernel(long long* __restrict__ sums, float* __restrict__ cent, long long count) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= count) return;
  long long s[6];
  for (int j = 0; j < 6; ++j) { s[j] = sums[i * 6 + j]; sums[i * 6 + j] = 0; }
  if (s[5] <= 0) return;                                        // no pixel: the centroid keeps its value
  const double cnt = (double)s[5];
  float* c = cent + i * 5;
  c[0] = (float)((double)s[0] / cnt); c[1] = (float)((double)s[1] / cnt);
  for (int j = 2; j < 5; ++j) c[j] = (float)((double)s[j] / (cnt * 16777216.0));
}

// ---- connectivity ----------------------------------------------------------------------------------------------------------

// members are the pixels inside the image, linked on equal labels (cc_inl.h); size, mark and misc are cleared on the way
__global__ __launch_bounds__(NT) void slic_label_tiles_kernel(const int* __restrict__ seg, int H, int W, int* __restrict__ parent,
                                                              int* __restrict__ size, unsigned char* __restrict__ mark, int* __restrict__ misc) {
  __shared__ int par[T * T];
  __shared__ int val[T * T];
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t HW = (size_t)H * W, base = (size_t)n * HW;
  if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    misc[1 + n] = 0;
    if (n == 0) misc[0] = 0;
  }
  for (int l = tid; l < T * T; l += NT) {
    const int y = y0 + l / T, x = x0 + l % T;
    if (y < H && x < W) {
      const size_t p = base + (size_t)y * W + x;
      val[l] = seg[p]; size[p] = 0; mark[p] = 0;
    }
  }
  __syncthreads();
  const auto same = [&](int a, int b) { return val[a] == val[b]; };
  for (int l = tid; l < T * T; l += NT) par[l] = cc_run_parent<T, NT>(l, y0 + l / T < H && x0 + l % T < W, same);
  __syncthreads();
  for (int l = tid; l < T * T; l += NT) cc_tile_unions<4, T>(par, l, same);
  __syncthreads();
  for (int l = tid; l < T * T; l += NT) {
    if (par[l] < 0) continue;
    parent[base + (size_t)(y0 + l / T) * W + (x0 + l % T)] = cc_tile_root<T>(par, l, base, y0, x0, W);
  }
}

__global__ __launch_bounds__(NT) void slic_join_tiles_kernel(const int* __restrict__ seg, int* parent, int N, int H, int W) {
  const long long total = (long long)N * H * W, p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  cc_join_borders<4, T>(parent, p, H, W, [](long long) { return true; }, [seg](long long a, long long b) { return seg[a] == seg[b]; });
}

__global__ __launch_bounds__(NT) void slic_flatten_kernel(int* parent, int* size, long long total) {
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  atomicAdd(size + cc_flatten(parent, p), 1);
}

// the breadth-first search of include/camo_slic.h step 8 for the small component whose first pixel is `root`: -> the root of the
// component whose label it adopts, or -1.  parent[] holds roots; a neighbour's component comes earlier when its root is smaller.
__device__ int slic_search(const int* __restrict__ parent, unsigned char* mark, int* qu, int root, int count, int base, int H, int W) {
  int head = 0, tail = 1, adjacent = -1;
  qu[0] = root; mark[root] = 1;
  while (head < tail) {
    const int c = qu[head++], q = c - base, y = q / W, x = q - y * W;
    for (int dir = 0; dir < 4; ++dir) {
      int nb;
      if (dir == 0) { if (x + 1 >= W) continue; nb = c + 1; }
      else if (dir == 1) { if (x < 1) continue; nb = c - 1; }
      else if (dir == 2) { if (y + 1 >= H) continue; nb = c + W; }
      else { if (y < 1) continue; nb = c - W; }
      const int r = parent[nb];
      if (r == root) {
        if (!mark[nb] && tail < count) { mark[nb] = 1; qu[tail++] = nb; }
      } else if (r < root) {
        adjacent = r;
      }
    }
  }
  return adjacent;
}

__global__ __launch_bounds__(NT) void slic_search_kernel(const int* __restrict__ parent, const int* __restrict__ size, int H, int W, int min_size,
                                                         int max_size, int* __restrict__ adj, int* queue, unsigned char* mark,
                                                         int* __restrict__ chunk, int* misc) {
  __shared__ int large, over;
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W, base = n * HW;
  if (tid == 0) { large = 0; over = 0; }
  __syncthreads();
  int nl = 0, no = 0;
  for (int j = 0; j < SLIC_CHUNK / NT; ++j) {
    const int q = blockIdx.x * SLIC_CHUNK + j * NT + tid;
    if (q >= HW) continue;
    const int p = base + q;
    if (parent[p] != p) continue;
    const int count = size[p];
    if (count >= min_size) {
      ++nl;
      if (count >= max_size) ++no;
    } else {
      int* qu = queue + atomicAdd(misc, count);                 // (the small components are disjoint: at most N H W entries in all)
      adj[p] = slic_search(parent, mark, qu, p, count, base, H, W);
    }
  }
  if (nl) atomicAdd(&large, nl);
  if (no) atomicAdd(&over, no);
  __syncthreads();
  if (tid == 0) {
    chunk[n * gridDim.x + blockIdx.x] = large;
    if (over) atomicAdd(misc + 1 + n, over);
  }
}

// one block per image: chunk[] becomes its exclusive prefix; counts = {large components + 1, oversized components}
__global__ __launch_bounds__(NT) void slic_scan_kernel(int* __restrict__ chunk, int chunks, const int* __restrict__ misc, int* __restrict__ counts) {
  __shared__ int s[NT];
  const int n = blockIdx.x;
  const int large = block_chunk_prefix<NT>(chunk + (size_t)n * chunks, chunks, s, [](int) {});
  if (threadIdx.x == 0) { counts[2 * n] = large + 1; counts[2 * n + 1] = misc[1 + n]; }
}

__global__ __launch_bounds__(NT) void slic_rank_kernel(const int* __restrict__ parent, const int* __restrict__ size, int H, int W, int min_size,
                                                       const int* __restrict__ chunk, int* __restrict__ adj) {
  __shared__ int wcount[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W, base = n * HW;
  int running = chunk[n * gridDim.x + blockIdx.x];
  for (int j = 0; j < SLIC_CHUNK / NT; ++j) {
    const int q = blockIdx.x * SLIC_CHUNK + j * NT + tid, p = base + q;
    const bool is_large = q < HW && parent[p] == p && size[p] >= min_size;
    int total;
    const int before = block_rank<NT>(is_large, wcount, total);
    if (is_large) adj[p] = running + before + 1;
    running += total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(NT) void slic_emit_kernel(const int* __restrict__ parent, const int* __restrict__ size, const int* __restrict__ adj,
                                                       int min_size, int* __restrict__ labels, long long total) {
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  int r = parent[p];
  while (r >= 0 && size[r] < min_size) r = adj[r];              // (adj[r] < r for a small component: the chain ends)
  labels[p] = r < 0 ? 0 : adj[r];
}

}  // namespace

SlicConnWs slic_conn_carve(int N, int H, int W, void* base) {
  SlicConnWs w{};
  camo_abi::Carver c(base);
  const size_t npix = (size_t)N * H * W, chunks = ((size_t)H * W + SLIC_CHUNK - 1) / SLIC_CHUNK;
  w.parent = c.take<int>(npix);
  w.size = c.take<int>(npix);
  w.adj = c.take<int>(npix);
  w.queue = c.take<int>(npix);
  w.mark = c.take<unsigned char>(npix);
  w.chunk = c.take<int>((size_t)N * chunks);
  w.misc = c.take<int>((size_t)N + 1);
  w.bytes = c.bytes();
  return w;
}

SlicWs slic_carve(int N, int H, int W, int K, void* base) {
  SlicWs w{};
  w.conn = slic_conn_carve(N, H, W, base);
  camo_abi::Carver c(base, w.conn.bytes);
  const size_t npix = (size_t)N * H * W;
  w.lab = c.take<float>(3 * npix);
  w.nearest = c.take<int>(npix);
  w.cent = c.take<float>((size_t)N * K * 5);
  w.sums = c.take<long long>((size_t)N * K * 6);
  w.bytes = c.bytes();
  return w;
}

static dim3 slic_tiles(int N, int H, int W) { return dim3((W + T - 1) / T, (H + T - 1) / T, N); }
static unsigned slic_blocks(long long count) { return (unsigned)((count + NT - 1) / NT); }

int launch_slic_preprocess(const float* images, int N, int H, int W, const CannyTaps& taps, float inv_compactness, float* lab, hipStream_t stream) {
  const int S = T + 2 * taps.radius;
  const size_t lds = ((size_t)S * S + (size_t)S * T + 3 * T * T) * sizeof(float);     // 60 KB at the largest radius
  hipLaunchKernelGGL(slic_preprocess_kernel, slic_tiles(N, H, W), dim3(NT), lds, stream, images, H, W, taps, inv_compactness, lab);
  return (int)hipGetLastError();
}

int launch_slic_init(const SlicGrid& g, int N, float* cent, long long* sums, hipStream_t stream) {
  hipLaunchKernelGGL(slic_init_kernel, dim3(slic_blocks((long long)N * g.K)), dim3(NT), 0, stream, g, N, cent, sums);
  return (int)hipGetLastError();
}

int launch_slic_assign(const float* lab, const float* cent, int N, int H, int W, int K, int step, int* nearest, float* dist, hipStream_t stream) {
  hipLaunchKernelGGL(slic_assign_kernel, slic_tiles(N, H, W), dim3(NT), 0, stream, lab, cent, H, W, K, step, nearest, dist);
  return (int)hipGetLastError();
}

int launch_slic_update(const float* lab, const int* nearest, int N, int H, int W, int K, long long* sums, float* cent, bool clear_first,
                       hipStream_t stream) {
  const long long nk = (long long)N * K;
  if (clear_first) hipLaunchKernelGGL(slic_clear_kernel, dim3(slic_blocks(nk * 6)), dim3(NT), 0, stream, sums, nk * 6);
  hipLaunchKernelGGL(slic_accumulate_kernel, slic_tiles(N, H, W), dim3(NT), 0, stream, lab, nearest, H, W, K,
                     reinterpret_cast<unsigned long long*>(sums));
  hipLaunchKernelGGL(slic_finalize_kernel, dim3(slic_blocks(nk)), dim3(NT), 0, stream, sums, cent, nk);
  return (int)hipGetLastError();
}

int launch_slic_connect(const int* labels_in, int N, int H, int W, int min_size, int max_size, const SlicConnWs& ws, int* labels, int* counts,
                        hipStream_t stream) {
  const long long total = (long long)N * H * W;
  const int chunks = (int)(((long long)H * W + SLIC_CHUNK - 1) / SLIC_CHUNK);
  const dim3 raster(chunks, N);
  hipLaunchKernelGGL(slic_label_tiles_kernel, slic_tiles(N, H, W), dim3(NT), 0, stream, labels_in, H, W, ws.parent, ws.size, ws.mark, ws.misc);
  hipLaunchKernelGGL(slic_join_tiles_kernel, dim3(slic_blocks(total)), dim3(NT), 0, stream, labels_in, ws.parent, N, H, W);
  hipLaunchKernelGGL(slic_flatten_kernel, dim3(slic_blocks(total)), dim3(NT), 0, stream, ws.parent, ws.size, total);
  hipLaunchKernelGGL(slic_search_kernel, raster, dim3(NT), 0, stream, ws.parent, ws.size, H, W, min_size, max_size, ws.adj, ws.queue, ws.mark,
                     ws.chunk, ws.misc);
  hipLaunchKernelGGL(slic_scan_kernel, dim3(N), dim3(NT), 0, stream, ws.chunk, chunks, ws.misc, counts);
  hipLaunchKernelGGL(slic_rank_kernel, raster, dim3(NT), 0, stream, ws.parent, ws.size, H, W, min_size, ws.chunk, ws.adj);
  hipLaunchKernelGGL(slic_emit_kernel, dim3(slic_blocks(total)), dim3(NT), 0, stream, ws.parent, ws.size, ws.adj, min_size, labels, total);
  return (int)hipGetLastError();
}
