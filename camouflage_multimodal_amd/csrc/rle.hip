// COCO run-length masks (include/camo_rle.h): label maps to runs along COCO's column-major order, and the counts of
// annotations to label maps.  Every grid covers the whole batch.
//
//   count    per 64 x 64 tile: the tile and the row above it go to LDS with lanes along x, come back with lanes along y; a ballot
//            counts the heads (positions whose label differs from the position before) of every column segment
//   scan     one block per image: exclusive prefix of the segment counts in column-major order (label_inl.h's label_scan), counts
//   emit     the count launch's tile body again: a head's rank is its segment's prefix plus the heads below it in the ballot;
//            (start, label) goes to row `rank`; the blocks of an image also zero the rows past its last run
//
//   prefix   one block per annotation: the start position of every run (64-bit prefix of the counts, clamped to H W), the sum and
//            the verdict; the blocks past the annotations clear the label maps
//   fill     16 lanes per count: binary search for the annotation, background counts leave, the lanes walk the positions (atomicMax)
//
// Integer arithmetic only; the one atomic is the 32-bit atomicMax of fill.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "common.h"
#include "label_inl.h"
#include "rle.h"
#include "../../include/camo_rle.h"

namespace {

constexpr int NT = 256, WAVES = NT / 64, TILE = RLE_TILE, LD = TILE + 1;      // LD: a wave reading a column touches 64 different banks
static_assert(TILE == 64, "a column segment is one wave's ballot");
constexpr int PREFIX_ITEMS = 8;          // counts a thread of the prefix launch sums before the block-wide scan: 2048 counts a pass
constexpr int FILL_GROUP = 16;           // lanes that share a count in the fill launch: a ground-truth run is tens of pixels, a noisy one 1 or 2
constexpr int FILL_PER_BLOCK = NT / FILL_GROUP;

// The tile body of the count and the emit launch, every thread of a block of NT calls.  tile: (TILE + 1) * LD ints of LDS; row 0 is
// the row above the tile -- for the image's first row the LAST row shifted one column right, which is where position p - 1 of a
// column's top pixel lies.  on_column(segment, ballot of the heads, head, p, label) runs in every lane of the wave that takes the
// column, lanes along y; segment = x * ceil(H / 64) + y / 64.
template <class OnColumn>
__device__ __forceinline__ void rle_tile(const int* __restrict__ img, int H, int W, int tx, int ty, int* tile, OnColumn on_column) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * TILE, y0 = ty * TILE, SH = (H + TILE - 1) / TILE;
  for (int r = wave; r <= TILE; r += WAVES) {
    int gy = y0 + r - 1, gx = x0 + lane;
    if (gy < 0) { gy = H - 1; gx -= 1; }                             // (r == 0 of the first tile row)
    int v = 0;
    if (gy < H && gx >= 0 && gx < W) v = img[(size_t)gy * W + gx];
    tile[r * LD + lane] = v;
  }
  __syncthreads();
  for (int c = wave; c < TILE && x0 + c < W; c += WAVES) {
    const int x = x0 + c, y = y0 + lane;
    const int v = tile[(lane + 1) * LD + c], before = tile[lane * LD + c];
    const int p = x * H + y;
    const bool head = y < H && (p == 0 || v != before);
    on_column(x * SH + ty, __ballot(head), head, p, v);
  }
}

// grid (tiles, images)
__global__ __launch_bounds__(NT) void rle_count_kernel(const int* __restrict__ labels, int H, int W, int tiles_x, int* __restrict__ seg) {
  __shared__ int tile[(TILE + 1) * LD];
  const int n = blockIdx.y, S = W * ((H + TILE - 1) / TILE);
  int* out = seg + (size_t)n * S;
  rle_tile(labels + (size_t)n * H * W, H, W, blockIdx.x % tiles_x, blockIdx.x / tiles_x, tile,
           [&](int s, unsigned long long heads, bool, int, int) {
             if ((threadIdx.x & 63) == 0) out[s] = __popcll(heads);
           });
}

// grid (images)
__global__ __launch_bounds__(NT) void rle_scan_kernel(const int* __restrict__ seg, int S, int R, int* __restrict__ pre, int* __restrict__ counts) {
  __shared__ int wsum[WAVES];
  const int n = blockIdx.x;
  const int M = label_scan<NT>(seg + (size_t)n * S, S, pre + (size_t)n * S, wsum);
  if (threadIdx.x == 0) { counts[2 * n] = M; counts[2 * n + 1] = min(M, R); }
}

// grid (tiles, images)
__global__ __launch_bounds__(NT) void rle_emit_kernel(const int* __restrict__ labels, int H, int W, int tiles_x, const int* __restrict__ pre, int R,
                                                      const int* __restrict__ counts, int* __restrict__ runs) {
  __shared__ int tile[(TILE + 1) * LD];
  const int n = blockIdx.y, S = W * ((H + TILE - 1) / TILE);
  const int* base = pre + (size_t)n * S;
  int2* rows = reinterpret_cast<int2*>(runs) + (size_t)n * R;
  rle_tile(labels + (size_t)n * H * W, H, W, blockIdx.x % tiles_x, blockIdx.x / tiles_x, tile,
           [&](int s, unsigned long long heads, bool head, int p, int v) {
             const int lane = threadIdx.x & 63;
             const int rank = base[s] + __popcll(heads & ((1ull << lane) - 1ull));
             if (head && rank < R) rows[rank] = make_int2(p, v);
           });
  const long long step = (long long)gridDim.x * NT;                 // the rows past the last run, shared among the image's blocks
  for (long long r = min(counts[2 * n], R) + (long long)blockIdx.x * NT + threadIdx.x; r < R; r += step) rows[r] = make_int2(0, 0);
}

// grid (annotations + clear blocks).  Block a < A: start[i] of annotation a's counts, ann_sum[a].  The others: labels to 0.
__global__ __launch_bounds__(NT) void rle_prefix_kernel(const int* __restrict__ cnts, int total, const int* __restrict__ ann_off,
                                                        const int* __restrict__ ann_image, const int* __restrict__ ann_value, int A, int N, int HW,
                                                        int* __restrict__ start, long long* __restrict__ ann_sum, int* __restrict__ labels,
                                                        long long pixels) {
  __shared__ long long wsum[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= A) {                                        // (the whole block)
    const long long step = (long long)(gridDim.x - A) * NT;
    for (long long i = (long long)(blockIdx.x - A) * NT + tid; i < pixels; i += step) labels[i] = 0;
    return;
  }
  const int a = blockIdx.x;
  const int lo = min(max(ann_off[a], 0), total), hi = min(max(ann_off[a + 1], lo), total);      // (inside cnts whatever ann_off holds)
  const bool valid = ann_image[a] >= 0 && ann_image[a] < N && ann_value[a] >= 1;
  long long carry = 0;
  bool negative = false;
  for (int c0 = lo; c0 < hi; c0 += NT * PREFIX_ITEMS) {              // a pass: PREFIX_ITEMS consecutive counts a thread
    const int i0 = c0 + tid * PREFIX_ITEMS;
    int v[PREFIX_ITEMS];
    long long sum = 0;
#pragma unroll
    for (int k = 0; k < PREFIX_ITEMS; ++k) {
      v[k] = i0 + k < hi ? cnts[i0 + k] : 0;
      negative |= v[k] < 0;
      sum += v[k];
    }
    const long long inc = wave_scan_ll(sum);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long at = carry + inc - sum;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      if (w < wave) at += wsum[w];
      carry += wsum[w];
    }
#pragma unroll
    for (int k = 0; k < PREFIX_ITEMS; ++k) {
      if (i0 + k < hi) start[i0 + k] = (int)min(max(at, 0ll), (long long)HW);
      at += v[k];
    }
    __syncthreads();
  }
  const int bad = __syncthreads_or(negative);
  if (tid == 0) ann_sum[a] = valid && !bad ? carry : -1;
}

// grid (counts / FILL_PER_BLOCK): FILL_GROUP consecutive lanes take count g
__global__ __launch_bounds__(NT) void rle_fill_kernel(const int* __restrict__ cnts, int total, const int* __restrict__ ann_off,
                                                      const int* __restrict__ ann_image, const int* __restrict__ ann_value, int A, int H, int W,
                                                      const int* __restrict__ start, const long long* __restrict__ ann_sum, int* __restrict__ labels) {
  const int sub = threadIdx.x % FILL_GROUP;
  const int g = blockIdx.x * FILL_PER_BLOCK + threadIdx.x / FILL_GROUP;
  if (g >= total) return;                                            // (the whole group, here and below; no cross-lane step follows)
  int lo = 0, hi = A - 1;                                            // the last annotation that starts at or before g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ann_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const int a = lo;
  if (((g - ann_off[a]) & 1) == 0) return;                           // a background count
  if (ann_sum[a] < 0) return;                                        // (so its image and value are in range and no count is negative)
  const int HW = H * W, s = start[g];
  if (s < 0 || s >= HW) return;
  const int e = (int)min((long long)s + cnts[g], (long long)HW);
  int* img = labels + (size_t)ann_image[a] * HW;
  const int v = ann_value[a];
  for (int p = s + sub; p < e; p += FILL_GROUP) {
    const int x = p / H, y = p - x * H;
    atomicMax(img + (size_t)y * W + x, v);
  }
}

}  // namespace

RleRunsWs rle_runs_carve(int N, int H, int W, void* base) {
  RleRunsWs w{};
  camo_abi::Carver c(base);
  const size_t S = (size_t)W * ((H + TILE - 1) / TILE);
  w.seg = c.take<int>((size_t)N * S);
  w.pre = c.take<int>((size_t)N * S);
  w.bytes = c.bytes();
  return w;
}

RleDecodeWs rle_decode_carve(int total, void* base) {
  RleDecodeWs w{};
  camo_abi::Carver c(base);
  w.start = c.take<int>((size_t)std::max(total, 1));
  w.bytes = c.bytes();
  return w;
}

int launch_rle_runs(const int* labels, int N, int H, int W, int R, const RleRunsWs& ws, int* runs, int* counts, hipStream_t stream) {
  const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE, S = W * tiles_y;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)N);
  hipLaunchKernelGGL(rle_count_kernel, grid, dim3(NT), 0, stream, labels, H, W, tiles_x, ws.seg);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(N), dim3(NT), 0, stream, ws.seg, S, R, ws.pre, counts);
  hipLaunchKernelGGL(rle_emit_kernel, grid, dim3(NT), 0, stream, labels, H, W, tiles_x, ws.pre, R, counts, runs);
  return (int)hipGetLastError();
}

int launch_rle_decode(const int* cnts, int total, const int* ann_off, const int* ann_image, const int* ann_value, int A, int N, int H, int W,
                      const RleDecodeWs& ws, int* labels, long long* ann_sum, hipStream_t stream) {
  const long long pixels = (long long)N * H * W;
  const unsigned clear_blocks = (unsigned)std::min<long long>((pixels + NT - 1) / NT, 4096);
  hipLaunchKernelGGL(rle_prefix_kernel, dim3(A + clear_blocks), dim3(NT), 0, stream, cnts, total, ann_off, ann_image, ann_value, A, N, H * W, ws.start,
                     ann_sum, labels, pixels);
  if (total > 0)
    hipLaunchKernelGGL(rle_fill_kernel, dim3((unsigned)((total + FILL_PER_BLOCK - 1) / FILL_PER_BLOCK)), dim3(NT), 0, stream, cnts, total, ann_off, ann_image, ann_value, A, H,
                       W, ws.start, ann_sum, labels);
  return (int)hipGetLastError();
}
