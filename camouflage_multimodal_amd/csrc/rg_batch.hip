// Region-graph construction for a whole batch of images (include/camo_rg_batch.h): what rg_features.hip computes for one image,
// for N label maps in one call and with integer sums, so that the result does not depend on the order the additions arrive in.
// SEVEN launches whatever N is; every grid covers the whole batch.
//
//   clear      zero the sums, the adjacency bits and status
//   accumulate one block per 32 x 32 tile of one image.  The tile's labels with a halo of 2 are staged in LDS (the 12
//              neighbour reads of a pixel are LDS reads); per-label sums go into an LDS hash table (keys[SLOTS], 64-bit integer
//              LDS atomics, the layout of slic_accumulate_kernel), then one 64-bit integer global atomic per occupied slot and
//              non-zero quantity.  A label that finds the table full adds to global memory directly: either way the same
//              integers reach the same sum.  Pixel p with label r:
//                own sums into acc[r]: count, RGB, luma (reals as v = llrint(q 2^36)), their squares v^2 exactly in two limbs, y, x, edge-map
//                perimeter[l] += 1 for every distinct label l != r among p's 4-neighbours      (|dilate(mask_l) xor mask_l| [:184])
//                ring sums of l (RGB, count) += p for every distinct l != r within L1 distance 2 (dilate(mask_l, iterations=2) & ~mask_l [:191-192])
//                adj bit (min, max) for every 8-neighbour label != r                             (RAG, connectivity 2 [:215])
//   rank       one block per image: compaction of the non-empty labels by ballot prefix (region_id_map [:231]) -> region_map, kept[n]
//   finalize   one lane per (image, label); the image's first row node_off[n] = sum of kept[0 .. n) is summed again by every
//              block (N small integers), so no block waits for another; 15 features per kept region [:201-212], batch, node_off
//   count      one wave per (image, label a): its neighbours b > a (a popcount of the row's bits)
//   scan       one block per image: exclusive prefix of the counts -> rowoff, pairs[n]
//   emit       one wave per (image, label a): edge_off[n] from pairs[0 .. n) likewise; its pairs (i, j), (j, i) as global node
//              indices with the weight [:226-234]
//
// A launch reads what an earlier launch of the same stream wrote: stream order makes that visible on every XCD, nothing else
// is needed.  Within accumulate, blocks meet only in relaxed agent-scope integer atomics (atomicAdd / atomicOr), whose results
// nobody reads before the launch ends.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "abi_util.h"
#include "label_inl.h"
#include "rg_batch.h"

namespace {

// (A_xx: the high limb of the sum of squares, in units of 2^-36 like the sums; A_xx_LO: the low limb, in units of 2^-72)
enum { A_CNT = 0, A_R, A_G, A_B, A_L, A_RR, A_GG, A_BB, A_LL, A_RR_LO, A_GG_LO, A_BB_LO, A_LL_LO, A_Y, A_X, A_E, A_PERIM, A_NR, A_NG, A_NB, A_NCNT };
constexpr int NOWN = A_E + 1;            // quantities a pixel adds to its own label
static_assert(A_NCNT + 1 == RGB_NACC, "accumulator layout");

constexpr int T = 32, NT = 256, PPT = T * T / NT, HALO = 2, LW = T + 2 * HALO;
constexpr int SLOTS = RGB_SLOTS;
constexpr double FIX = 68719476736.0, UNIT = 1.0 / 68719476736.0;      // 2^36, 2^-36
static_assert(RGB_FIX_BITS == 36, "FIX is 2^RGB_FIX_BITS");

typedef unsigned long long u64;

__global__ __launch_bounds__(NT) void rgb_clear_kernel(u64* acc, size_t nacc, unsigned int* adj, size_t nwords, int* status) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x, stride = (size_t)gridDim.x * NT;
  for (size_t k = i; k < nacc; k += stride) acc[k] = 0;
  for (size_t k = i; k < nwords; k += stride) adj[k] = 0u;
  if (i < 2) status[i] = 0;
}

__global__ __launch_bounds__(NT) void rgb_accumulate_kernel(const float* __restrict__ images, const int* __restrict__ seg,
                                                            const unsigned char* __restrict__ canny, int H, int W, int label_bound,
                                                            int words, u64* acc, unsigned int* adj, int* status) {
  // (rows of 36 labels: a wave reads 32 consecutive entries per half, and ds_read_b32 banks conflict within a half only)
  __shared__ int lab[LW * LW];
  __shared__ int keys[SLOTS];
  __shared__ u64 tab[SLOTS][RGB_NACC];
  __shared__ int bad;
  const int tid = threadIdx.x, n = blockIdx.z, ty0 = blockIdx.y * T, tx0 = blockIdx.x * T;
  const size_t HW = (size_t)H * W, base = (size_t)n * HW;
  for (int i = tid; i < SLOTS; i += NT) keys[i] = -1;
  for (int i = tid; i < SLOTS * RGB_NACC; i += NT) tab[i / RGB_NACC][i % RGB_NACC] = 0;
  if (tid == 0) bad = 0;
  __syncthreads();
  int nbad = 0;
  for (int i = tid; i < LW * LW; i += NT) {
    const int ly = i / LW, lx = i - ly * LW, y = ty0 - HALO + ly, x = tx0 - HALO + lx;
    int l = -1;                                                   // outside the image, or a label outside [0, label_bound)
    if (y >= 0 && y < H && x >= 0 && x < W) {
      l = seg[base + (size_t)y * W + x];
      if ((unsigned)l >= (unsigned)label_bound) {
        l = -1;
        if (ly >= HALO && ly < HALO + T && lx >= HALO && lx < HALO + T) ++nbad;   // (counted by the tile that owns the pixel)
      }
    }
    lab[i] = l;
  }
  if (nbad) atomicAdd(&bad, nbad);
  __syncthreads();
  u64* accn = acc + (size_t)n * label_bound * RGB_NACC;
  unsigned int* adjn = adj + (size_t)n * label_bound * words;
  for (int j = 0; j < PPT; ++j) {
    const int t = tid + j * NT, ly = t / T, lx = t - ly * T, y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    const int* c = lab + (ly + HALO) * LW + (lx + HALO);
    const int r = c[0];
    if (r < 0) continue;
    const size_t p = base + (size_t)y * W + x;
    const double cr = images[3 * p], cg = images[3 * p + 1], cb = images[3 * p + 2];
    const double luma = cr * 0.2989 + cg * 0.5870 + cb * 0.1140;  // np.dot(image, [0.2989, 0.5870, 0.1140]) [:151]
    const long long vr = llrint(cr * FIX), vg = llrint(cg * FIX), vb = llrint(cb * FIX), vl = llrint(luma * FIX);
    {
      // squares of the INTEGERS, exactly: v^2 < 2^73 as two limbs of 36 bits, each summed on its own (< 2^62 over 2^26 pixels)
      const unsigned __int128 sr = (unsigned __int128)((__int128)vr * vr), sg = (unsigned __int128)((__int128)vg * vg),
                              sb = (unsigned __int128)((__int128)vb * vb), sl = (unsigned __int128)((__int128)vl * vl);
      const u64 LO = (1ull << RGB_FIX_BITS) - 1;
      const long long val[NOWN] = {1, vr, vg, vb, vl, (long long)(sr >> RGB_FIX_BITS), (long long)(sg >> RGB_FIX_BITS), (long long)(sb >> RGB_FIX_BITS),
                                   (long long)(sl >> RGB_FIX_BITS), (long long)((u64)sr & LO), (long long)((u64)sg & LO), (long long)((u64)sb & LO),
                                   (long long)((u64)sl & LO), y, x, canny[p] ? 1 : 0};
      const int s = label_slot<SLOTS>(keys, r);
      if (s >= 0) {
#pragma unroll
        for (int q = 0; q < NOWN; ++q) if (val[q]) atomicAdd(&tab[s][q], (u64)val[q]);
      } else {
        u64* a = accn + (size_t)r * RGB_NACC;
#pragma unroll
        for (int q = 0; q < NOWN; ++q) if (val[q]) atomicAdd(a + q, (u64)val[q]);
      }
    }
    rg_visit_neighbours(
        r, [&](int ddy, int ddx) { return c[ddy * LW + ddx]; },    // (-1 outside the image: the halo holds it)
        [&](int l) {
          if (l < r) return;                                        // The neighbour sees this pixel in ITS 8-neighbourhood, so the
          unsigned int* w = adjn + (size_t)r * words + (l >> 5);    // pixel with the smaller label sets the bit of (min, max)
          const unsigned int bit = 1u << (l & 31);
          if (!(*w & bit)) atomicOr(w, bit);                        // (a stale 0 only repeats the atomic; the bits were cleared by an earlier launch)
        },
        [&](int l, bool four) {
          const long long val[5] = {four ? 1 : 0, vr, vg, vb, 1};
          const int s = label_slot<SLOTS>(keys, l);
          if (s >= 0) {
#pragma unroll
            for (int q = 0; q < 5; ++q) if (val[q]) atomicAdd(&tab[s][A_PERIM + q], (u64)val[q]);
          } else {
            u64* b = accn + (size_t)l * RGB_NACC + A_PERIM;
#pragma unroll
            for (int q = 0; q < 5; ++q) if (val[q]) atomicAdd(b + q, (u64)val[q]);
          }
        });
  }
  __syncthreads();
  for (int i = tid; i < SLOTS * RGB_NACC; i += NT) {
    const int k = keys[i / RGB_NACC];
    const u64 v = tab[i / RGB_NACC][i % RGB_NACC];
    if (k >= 0 && v) atomicAdd(accn + (size_t)k * RGB_NACC + i % RGB_NACC, v);
  }
  if (tid == 0 && bad) atomicAdd(status, bad);
}

// one block of 1024 threads per image; label_bound <= 4096
__global__ __launch_bounds__(1024) void rgb_rank_kernel(const u64* __restrict__ acc, int label_bound, int* __restrict__ region_map,
                                                        int* __restrict__ kept) {
  __shared__ int wsum[16];
  const int n = blockIdx.x;
  const u64* accn = acc + (size_t)n * label_bound * RGB_NACC;
  int* rmap = region_map + (size_t)n * label_bound;
  const int total = label_compact<1024>(
      label_bound, wsum, [&](int r) { return accn[(size_t)r * RGB_NACC + A_CNT] > 0; }, [&](int r, int rank) { rmap[r] = rank; });
  if (threadIdx.x == 0) kept[n] = total;
}

// sum of v[0 .. n) over the block's NT threads, the same value in every thread
__device__ __forceinline__ int rgb_block_prefix(const int* __restrict__ v, int n, int* red) {
  const int tid = threadIdx.x;
  int s = 0;
  for (int i = tid; i < n; i += NT) s += v[i];
  s = wave_sum_int(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// population variance of the fixed-point values from their integer sums: (n sum v^2 - (sum v)^2) / n^2, the numerator exactly in
// 128-bit integers (n <= 2^26, sum v^2 < 2^99, (sum v)^2 < 2^124), so a region of one flat colour has variance exactly 0
__device__ __forceinline__ double rgb_variance(u64 n, u64 sum, u64 sq_hi, u64 sq_lo) {
  const unsigned __int128 sq = ((unsigned __int128)sq_hi << RGB_FIX_BITS) + sq_lo;
  const unsigned __int128 num = (unsigned __int128)n * sq - (unsigned __int128)sum * sum;      // >= 0 (Cauchy-Schwarz)
  const double d = (double)(u64)(num >> 64) * 18446744073709551616.0 + (double)(u64)num;
  const double inv = 1.0 / (double)n;
  return d * inv * inv * UNIT * UNIT;
}

__global__ __launch_bounds__(NT) void rgb_finalize_kernel(const u64* __restrict__ acc, const int* __restrict__ region_map,
                                                          const int* __restrict__ kept, int N, int label_bound, float* __restrict__ x,
                                                          int* __restrict__ batch, int* __restrict__ node_off) {
  __shared__ int red[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.y, r = blockIdx.x * NT + tid;
  const int first = rgb_block_prefix(kept, n, red);
  if (blockIdx.x == 0 && tid == 0) {
    node_off[n] = first;
    if (n == N - 1) node_off[N] = first + kept[n];
  }
  if (r >= label_bound) return;
  const int rank = region_map[(size_t)n * label_bound + r];
  if (rank < 0) return;
  const u64* a = acc + ((size_t)n * label_bound + r) * RGB_NACC;
  // the sums as the reals they stand for, then the reference's formulas in double in this one order
  const double cnt = (double)a[A_CNT], inv = 1.0 / cnt;
  const double sr = (double)(long long)a[A_R] * UNIT, sg = (double)(long long)a[A_G] * UNIT, sb = (double)(long long)a[A_B] * UNIT;
  const double sl = (double)(long long)a[A_L] * UNIT;
  const double mr = sr * inv, mg = sg * inv, mb = sb * inv, ml = sl * inv;
  const double vr = rgb_variance(a[A_CNT], a[A_R], a[A_RR], a[A_RR_LO]), vg = rgb_variance(a[A_CNT], a[A_G], a[A_GG], a[A_GG_LO]),
               vb = rgb_variance(a[A_CNT], a[A_B], a[A_BB], a[A_BB_LO]), vl = rgb_variance(a[A_CNT], a[A_L], a[A_LL], a[A_LL_LO]);
  double contrast = 0.0;
  if (a[A_NCNT] > 0) {
    const double q = 1.0 / (double)a[A_NCNT];
    const double d0 = mr - (double)(long long)a[A_NR] * UNIT * q, d1 = mg - (double)(long long)a[A_NG] * UNIT * q,
                 d2 = mb - (double)(long long)a[A_NB] * UNIT * q;
    contrast = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  }
  rg_store_features(x + (size_t)(first + rank) * RGF_NFEAT, {mr, mg, mb, ml, vr, vg, vb, vl, (double)a[A_X] * inv, (double)a[A_Y] * inv, cnt,
                                                             (double)a[A_PERIM], contrast, (double)a[A_E] * inv});
  batch[first + rank] = n;
}

// one wave per (image, label a).  A bit of row a stands for a label b > a, set by a pixel of a beside a pixel of b: both labels
// have pixels, so both are kept, and the row's popcount is the number of a's edges
__global__ __launch_bounds__(NT) void rgb_count_kernel(const unsigned int* __restrict__ adj, int label_bound, int words, int* __restrict__ rowcount) {
  const int lane = threadIdx.x & 63, a = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), n = blockIdx.y;
  if (a >= label_bound) return;
  const unsigned int* row = adj + ((size_t)n * label_bound + a) * words;
  int c = 0;
  for (int w = lane; w < words; w += 64) c += __popc(row[w]);
  c = wave_sum_int(c);
  if (lane == 0) rowcount[(size_t)n * label_bound + a] = c;
}

// one block per image
__global__ __launch_bounds__(1024) void rgb_scan_kernel(const int* __restrict__ rowcount, int label_bound, int* __restrict__ rowoff,
                                                        int* __restrict__ pairs) {
  __shared__ int wsum[16];
  const size_t row = (size_t)blockIdx.x * label_bound;
  const int total = label_scan<1024>(rowcount + row, label_bound, rowoff + row, wsum);
  if (threadIdx.x == 0) pairs[blockIdx.x] = total;
}

// one wave per (image, label a): its neighbours b > a in increasing order
__global__ __launch_bounds__(64) void rgb_emit_kernel(const unsigned int* __restrict__ adj, const int* __restrict__ region_map,
                                                      const int* __restrict__ rowoff, const int* __restrict__ pairs,
                                                      const int* __restrict__ node_off, const float* __restrict__ x, int N, int label_bound,
                                                      int words, long long* __restrict__ edge_index, float* __restrict__ edge_attr,
                                                      int edge_capacity, int* __restrict__ edge_off, int* __restrict__ status) {
  const int a = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  int before = 0;                                               // undirected edges of the images in front of this one
  for (int i = lane; i < n; i += 64) before += pairs[i];
  before = wave_sum_int(before);
  if (a == 0 && lane == 0) {
    edge_off[n] = 2 * before;
    if (n == N - 1) { edge_off[N] = 2 * (before + pairs[n]); status[1] = 2 * (before + pairs[n]); }
  }
  const int* rmap = region_map + (size_t)n * label_bound;
  if (rmap[a] < 0) return;
  const int first = node_off[n];
  const unsigned int* row = adj + ((size_t)n * label_bound + a) * words;
  rg_emit_row(
      a, label_bound, before + rowoff[(size_t)n * label_bound + a], first + rmap[a], x,
      [&](int b) { return ((row[b >> 5] >> (b & 31)) & 1u) && rmap[b] >= 0; }, [&](int b) { return first + rmap[b]; }, edge_index, edge_attr,
      edge_capacity);
}

}  // namespace

RgBatchWs rg_batch_carve(int N, int label_bound, void* base) {
  RgBatchWs w{};
  camo_abi::Carver c(base);
  const size_t nl = (size_t)N * label_bound;
  w.words = (label_bound + 31) / 32;
  w.acc = c.take<unsigned long long>(nl * RGB_NACC);
  w.adj = c.take<unsigned int>(nl * w.words);
  w.kept = c.take<int>((size_t)N);
  w.rowcount = c.take<int>(nl);
  w.rowoff = c.take<int>(nl);
  w.pairs = c.take<int>((size_t)N);
  w.bytes = c.bytes();
  return w;
}

int launch_region_graph_batch(const float* images, const int* segments, const unsigned char* canny, int N, int H, int W, int label_bound,
                              const RgBatchWs& ws, float* x, int* region_map, long long* edge_index, float* edge_attr, int edge_capacity,
                              int* node_off, int* edge_off, int* batch, int* status, hipStream_t stream) {
  const size_t nl = (size_t)N * label_bound, nacc = nl * RGB_NACC, nwords = nl * ws.words;
  const unsigned clear_blocks = (unsigned)std::min<size_t>((std::max(nacc, nwords) + NT - 1) / NT, 2048);
  const unsigned lblocks = (unsigned)((label_bound + NT - 1) / NT), wblocks = (unsigned)((label_bound + NT / 64 - 1) / (NT / 64));
  hipLaunchKernelGGL(rgb_clear_kernel, dim3(clear_blocks), dim3(NT), 0, stream, ws.acc, nacc, ws.adj, nwords, status);
  hipLaunchKernelGGL(rgb_accumulate_kernel, dim3((W + T - 1) / T, (H + T - 1) / T, N), dim3(NT), 0, stream, images, segments, canny, H, W,
                     label_bound, ws.words, ws.acc, ws.adj, status);
  hipLaunchKernelGGL(rgb_rank_kernel, dim3(N), dim3(1024), 0, stream, ws.acc, label_bound, region_map, ws.kept);
  hipLaunchKernelGGL(rgb_finalize_kernel, dim3(lblocks, N), dim3(NT), 0, stream, ws.acc, region_map, ws.kept, N, label_bound, x, batch, node_off);
  hipLaunchKernelGGL(rgb_count_kernel, dim3(wblocks, N), dim3(NT), 0, stream, ws.adj, label_bound, ws.words, ws.rowcount);
  hipLaunchKernelGGL(rgb_scan_kernel, dim3(N), dim3(1024), 0, stream, ws.rowcount, label_bound, ws.rowoff, ws.pairs);
  hipLaunchKernelGGL(rgb_emit_kernel, dim3(label_bound, N), dim3(64), 0, stream, ws.adj, region_map, ws.rowoff, ws.pairs, node_off, x, N,
                     label_bound, ws.words, edge_index, edge_attr, edge_capacity, edge_off, status);
  return (int)hipGetLastError();
}
