// Camouflaged-object benchmark measures (include/camo_seg_measures.h): the per-image histogram table behind S-alpha,
// E-phi and the F-beta curve, and the sums behind the weighted F-measure.  Integer sums only: every output is a function of the inputs.
// The C entry points stand at the end of the file; all argument checks run there, before any launch.
#include "seg_measures.h"

#include <algorithm>

#include "abi_util.h"
#include "../../include/camo_seg_measures.h"

using namespace camo_abi;

namespace {

constexpr int NT = SEGM_NT;
constexpr int HIST = CAMO_SEG_HIST_INTS;
constexpr unsigned NO_KEY = 0xFFFFu;         // key of an element outside the image: never added
static_assert(HIST == CAMO_SEG_QUADRANTS * 2 * CAMO_SEG_BINS && CAMO_SEG_BINS == 256, "a key is quadrant * 512 + g * 256 + q");
static_assert(SEGM_SPAN == 16, "a span is four float4 loads");

// rint(a / b) of the exact rational, a half to the even neighbour (a >= 0, b >= 1)
__device__ __forceinline__ long long rint_div(unsigned long long a, unsigned long long b) {
  const unsigned long long q = a / b, r = a - q * b;
  return (long long)(2 * r > b ? q + 1 : 2 * r == b ? q + (q & 1) : q);
}

__global__ void segm_clear_kernel(int* __restrict__ a, long long na, int* __restrict__ b, long long nb) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < na) a[i] = 0;
  else if (i - na < nb) b[i - na] = 0;
}

// four consecutive bytes of g starting at any address, from the one or two aligned words that hold them (the second word is read
// only when it holds one of the four)
__device__ __forceinline__ unsigned load_bytes4(const unsigned char* g) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(g);
  const unsigned* w = reinterpret_cast<const unsigned*>(a & ~(uintptr_t)3);
  const unsigned sh = (unsigned)(a & 3);
  const unsigned lo = w[0], hi = sh ? w[1] : 0u;
  return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * sh));
}

// grid (blocks per image, N).  A lane takes 16 bytes of gt at a time (one aligned 16-byte load inside the image, single bytes at
// its two ends) and adds, per positive pixel, 1 | x | y.  Lane -> wave -> block (LDS) -> three 64-bit integer atomics per block
// into the first 24 bytes of the image's table; the block that draws the image's last ticket (split[2 i], cleared before) reads the
// three sums back, writes the split point and clears the 24 bytes for the fill.
__global__ __launch_bounds__(NT) void segm_centroid_kernel(const unsigned char* __restrict__ gt, int H, int W, int* __restrict__ hist,
                                                           int* __restrict__ split) {
  __shared__ unsigned long long blk[3];
  const int i = blockIdx.y, tid = threadIdx.x, HW = H * W;
  const unsigned char* g = gt + (size_t)i * HW;
  const int a = (int)(reinterpret_cast<uintptr_t>(g) & 15);
  const int nchunks = (HW + a + 15) / 16;
  if (tid < 3) blk[tid] = 0ull;
  __syncthreads();
  unsigned n = 0;
  unsigned long long sx = 0, sy = 0;
  for (int c = blockIdx.x * NT + tid; c < nchunks; c += gridDim.x * NT) {
    const int q0 = c * 16 - a;
    unsigned m = 0;                                  // bit j: pixel q0 + j is positive
    if (q0 >= 0 && q0 + 16 <= HW) {
      const uint4 v = *reinterpret_cast<const uint4*>(g + q0);
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b) m |= ((w[k] >> (8 * b + 7)) & 1u) << (4 * k + b);
    } else {
      for (int j = 0; j < 16; ++j) {
        const int q = q0 + j;
        if (q >= 0 && q < HW && g[q] > 127) m |= 1u << j;
      }
    }
    while (m) {
      const int j = __ffs((int)m) - 1;
      m &= m - 1;
      const int q = q0 + j, y = q / W;
      ++n; sx += (unsigned)(q - y * W); sy += (unsigned)y;
    }
  }
  n = wave_sum_u32(n); sx = wave_sum_u64(sx); sy = wave_sum_u64(sy);
  if ((tid & 63) == 0 && n) { atomicAdd(&blk[0], (unsigned long long)n); atomicAdd(&blk[1], sx); atomicAdd(&blk[2], sy); }
  __syncthreads();
  if (tid != 0) return;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(hist + (size_t)i * HIST);
  if (blk[0]) { atomicAdd(acc + 0, blk[0]); atomicAdd(acc + 1, blk[1]); atomicAdd(acc + 2, blk[2]); }
  __threadfence();                                   // the three adds are performed before the ticket is drawn
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned ticket = atomicAdd(reinterpret_cast<unsigned*>(split) + 2 * i, 1u);
  if (ticket != gridDim.x - 1) return;
  __threadfence();
  const unsigned long long nf = __hip_atomic_load(acc + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long fx = __hip_atomic_load(acc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long fy = __hip_atomic_load(acc + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const long long cx = nf ? rint_div(fx, nf) : rint_div((unsigned long long)W, 2ull);
  const long long cy = nf ? rint_div(fy, nf) : rint_div((unsigned long long)H, 2ull);
  acc[0] = 0ull; acc[1] = 0ull; acc[2] = 0ull;
  split[2 * i] = (int)cx + 1;
  split[2 * i + 1] = (int)cy + 1;
}

// grid (blocks per image, N).  One histogram of 4 * 2 * 256 int32 per WAVE in LDS (32 KB a block).  A lane takes a span of 16
// consecutive pixels -- four aligned float4 loads of pred and the 16 bytes of gt beside them -- and walks its 16 keys in registers:
// equal consecutive keys become one (key, count) pair, so a painted (piecewise-constant) map costs a lane one or two LDS atomics a
// span instead of 16.  Where SEGM_UNIFORM_LANES or more lanes of the wave flush the SAME key in the same step (a saturated map: all 64),
// their counts are summed with shuffles and one lane adds the total: the 64 same-address LDS atomics that would be serialised do
// not happen.  The block adds its non-zero bins to the image's table with 32-bit integer atomics, once.
__global__ __launch_bounds__(NT) void segm_fill_kernel(const float* __restrict__ pred, long long stride, const unsigned char* __restrict__ gt,
                                                       int H, int W, const int* __restrict__ split, int* __restrict__ hist) {
  __shared__ unsigned lds[(NT / 64) * HIST];
  const int i = blockIdx.y, tid = threadIdx.x, lane = tid & 63, HW = H * W;
  const float* p = pred + (size_t)i * stride;
  const unsigned char* g = gt + (size_t)i * HW;
  unsigned* wh = lds + (tid >> 6) * HIST;
  const int X = split[2 * i], Y = split[2 * i + 1];
  const int a = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);      // p - a is 16-byte aligned
  const int nspans = (HW + a + SEGM_SPAN - 1) / SEGM_SPAN;
  for (int b = tid; b < (NT / 64) * HIST; b += NT) lds[b] = 0u;
  __syncthreads();

  for (int base = blockIdx.x * NT; base < nspans; base += gridDim.x * NT) {      // (the same trip count in every lane of the block)
    const int span = base + tid;
    unsigned k[SEGM_SPAN];
#pragma unroll
    for (int j = 0; j < SEGM_SPAN; ++j) k[j] = NO_KEY;
    if (span < nspans) {
      const int qs = span * SEGM_SPAN - a;                                        // (negative in span 0 only: -3 at the least)
      int y = qs > 0 ? qs / W : 0, x = qs - y * W;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int q0 = qs + 4 * c;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned gb = 0;
        const bool whole = q0 >= 0 && q0 + 4 <= HW;
        if (whole) {
          const float4 f = *reinterpret_cast<const float4*>(p + q0);
          v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
          gb = load_bytes4(g + q0);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (q0 + e >= 0 && q0 + e < HW) { v[e] = p[q0 + e]; gb |= (unsigned)g[q0 + e] << (8 * e); }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in = whole || (q0 + e >= 0 && q0 + e < HW);
          const unsigned quad = ((unsigned)(y >= Y) << 1) | (unsigned)(x >= X);
          const unsigned key = quad * 512u + (((gb >> (8 * e)) & 255u) > 127u ? 256u : 0u) + (unsigned)quantise_u8(v[e]);
          k[4 * c + e] = in ? key : NO_KEY;
          if (++x == W) { x = 0; ++y; }
        }
      }
    }
    unsigned cnt = 1;
#pragma unroll
    for (int j = 0; j < SEGM_SPAN; ++j) {
      const bool last = j == SEGM_SPAN - 1 || k[j + (j < SEGM_SPAN - 1)] != k[j];
      const bool flush = last && k[j] != NO_KEY;
      const unsigned long long fm = __ballot(flush);
      if (fm) {                                                                   // (wave-uniform)
        const int leader = __ffsll((long long)fm) - 1;
        const unsigned lk = (unsigned)__shfl((int)k[j], leader, 64);
        const bool same = flush && k[j] == lk;
        if (__popcll(__ballot(same)) >= SEGM_UNIFORM_LANES) {
          const unsigned total = wave_sum_u32(same ? cnt : 0u);
          if (lane == leader) atomicAdd(&wh[lk], total);
          else if (flush && !same) atomicAdd(&wh[k[j]], cnt);
        } else if (flush) {
          atomicAdd(&wh[k[j]], cnt);
        }
      }
      cnt = last ? 1u : cnt + 1u;
    }
  }
  __syncthreads();
  int* out = hist + (size_t)i * HIST;
  for (int b = tid; b < HIST; b += NT) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += lds[w * HIST + b];
    if (s) atomicAdd(out + b, (int)s);
  }
}

// ---- weighted F-measure ------------------------------------------------------------------------------------------------------

// grid (columns / NT, N): a thread scans its column down (the last positive row at or above y) and up (the first at or below y)
// and keeps the nearer one, a tie to the smaller row; -1 where the column has no positive pixel.
__global__ __launch_bounds__(NT) void segm_wf_column_kernel(const unsigned char* __restrict__ gt, int H, int W, int* __restrict__ ny) {
  const int i = blockIdx.y, x = blockIdx.x * NT + threadIdx.x;
  if (x >= W) return;
  const unsigned char* g = gt + (size_t)i * H * W;
  int* out = ny + (size_t)i * H * W;
  int above = -1;
  for (int y = 0; y < H; ++y) {
    if (g[(size_t)y * W + x] > 127) above = y;
    out[(size_t)y * W + x] = above;
  }
  int below = -1;
  for (int y = H - 1; y >= 0; --y) {
    if (g[(size_t)y * W + x] > 127) below = y;
    const int up = out[(size_t)y * W + x];
    out[(size_t)y * W + x] = up < 0 ? below : below < 0 ? up : (y - up <= below - y ? up : below);
  }
}

// grid (H, N): a block takes one row.  The row of nearest positive rows is staged in LDS; a thread then minimises
// (x - x')^2 + (y - y'(x'))^2 over x' in increasing order, keeping on a tie the candidate of the smaller y' (and so, for equal y',
// the smaller x').  The row is overwritten in place with d2 (0 on a positive pixel, -1 when the image has no positive pixel) and
// src receives the quantised prediction of the nearest positive pixel (its own on a positive pixel).
__global__ __launch_bounds__(NT) void segm_wf_row_kernel(const float* __restrict__ pred, long long stride, int H, int W, int* __restrict__ ny,
                                                         unsigned char* __restrict__ src) {
  __shared__ int row[CAMO_SEG_WF_MAX_SIDE];
  const int i = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
  const float* p = pred + (size_t)i * stride;
  int* d = ny + ((size_t)i * H + y) * W;
  unsigned char* s = src + ((size_t)i * H + y) * W;
  for (int x = tid; x < W; x += NT) row[x] = d[x];
  __syncthreads();
  for (int x = tid; x < W; x += NT) {
    int best = 0x7fffffff, by = -1, bx = -1;
    if (row[x] == y) {
      best = 0; by = y; bx = x;
    } else {
      for (int xx = 0; xx < W; ++xx) {
        const int yy = row[xx];
        if (yy < 0) continue;
        const int dy = y - yy, dx = x - xx, d2 = dy * dy + dx * dx;
        if (d2 < best || (d2 == best && yy < by)) { best = d2; by = yy; bx = xx; }
      }
    }
    d[x] = by < 0 ? -1 : best;
    s[x] = by < 0 ? (unsigned char)0 : (unsigned char)quantise_u8(p[(size_t)by * W + bx]);
  }
}

// grid (W / 32, H / 8, N), block 32 x 8.  Et of the tile and its halo of 3 is staged in LDS as doubles (zero outside the image);
// a positive pixel takes the 49 taps, a background pixel its weight; block-level integer sums, three 64-bit atomics per block.
__global__ __launch_bounds__(NT) void segm_wf_weight_kernel(const float* __restrict__ pred, long long stride, const unsigned char* __restrict__ gt,
                                                            int H, int W, const double* __restrict__ gauss, const int* __restrict__ d2,
                                                            const unsigned char* __restrict__ src, unsigned long long* __restrict__ sums) {
  constexpr int TX = SEGM_WF_TILE_X, TY = SEGM_WF_TILE_Y, LX = TX + 6, LY = TY + 6;
  static_assert(TX * TY == NT, "one thread per pixel of the tile");
  __shared__ double et[LY * LX];
  __shared__ double gk[49];
  __shared__ unsigned long long blk[3];
  const int i = blockIdx.z, tid = threadIdx.x, tx = tid % TX, ty = tid / TX;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)i * H * W;
  if (tid < 49) gk[tid] = gauss[tid];
  if (tid < 3) blk[tid] = 0ull;
  for (int idx = tid; idx < LX * LY; idx += NT) {
    const int gy = y0 + idx / LX - 3, gx = x0 + idx % LX - 3;
    et[idx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? fabs((double)src[plane + (size_t)gy * W + gx] / 255.0 - 1.0) : 0.0;
  }
  __syncthreads();
  const int x = x0 + tx, y = y0 + ty;
  unsigned nf = 0;
  unsigned long long afg = 0, abg = 0;
  if (x < W && y < H) {
    const size_t q = (size_t)y * W + x;
    const bool pos = gt[plane + q] > 127;
    const double e = fabs((double)quantise_u8(pred[(size_t)i * stride + q]) / 255.0 - (pos ? 1.0 : 0.0));
    if (pos) {
      double ea = 0.0;
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int c = 0; c < 7; ++c) ea += gk[j * 7 + c] * et[(ty + j) * LX + tx + c];
      nf = 1;
      afg = (unsigned long long)llrint(fmin(e, ea) * 4294967296.0);
    } else {
      const int dd = d2[plane + q];
      if (dd >= 0) {
        const double bw = 2.0 - exp(-0.6931471805599453 / 5.0 * sqrt((double)dd));
        abg = (unsigned long long)llrint(e * bw * 4294967296.0);
      }
    }
  }
  nf = wave_sum_u32(nf); afg = wave_sum_u64(afg); abg = wave_sum_u64(abg);
  if ((tid & 63) == 0) { atomicAdd(&blk[0], (unsigned long long)nf); atomicAdd(&blk[1], afg); atomicAdd(&blk[2], abg); }
  __syncthreads();
  if (tid < 3 && blk[tid]) atomicAdd(sums + (size_t)i * 3 + tid, blk[tid]);
}

struct WfWs { int* d2; unsigned char* src; size_t bytes; };
WfWs wf_carve(int N, int H, int W, void* base) {
  WfWs w{};
  Carver c(base);
  const size_t px = (size_t)N * H * W;
  w.d2 = c.take<int>(px);
  w.src = c.take<unsigned char>(px);
  w.bytes = c.bytes();
  return w;
}

int segm_check(const void* pred, long long stride, const void* gt, int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(CAMO_E_ARG, "need N >= 1, H >= 1, W >= 1");
  if (N > CAMO_RGD_MAX_IMAGES) return fail(CAMO_E_ARG, "N exceeds CAMO_RGD_MAX_IMAGES");
  if ((long long)H * W < 2) return fail(CAMO_E_ARG, "need H * W >= 2 (the measures divide by H * W - 1)");
  if ((long long)H * W > CAMO_RGD_MAX_IMAGE_PIXELS) return fail(CAMO_E_ARG, "H * W exceeds CAMO_RGD_MAX_IMAGE_PIXELS");
  if (stride < (long long)H * W) return fail(CAMO_E_ARG, "pred_image_stride must be >= H * W");
  if (!pred || !gt) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(pred) & 3) return fail(CAMO_E_ARG, "pred must be 4-byte aligned");
  return 0;
}

}  // namespace

extern "C" {

int camo_seg_histograms(const float* pred, int64_t pred_image_stride, const uint8_t* gt, int32_t N, int32_t H, int32_t W, int32_t* hist,
                        int32_t* split, void* stream) {
  if (int e = segm_check(pred, pred_image_stride, gt, N, H, W)) return e;
  if (!hist || !split) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(hist) & 7) return fail(CAMO_E_ARG, "hist must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(split) & 3) return fail(CAMO_E_ARG, "split must be 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int HW = H * W;
  const long long nh = (long long)N * HIST, ns = 2ll * N;
  hipLaunchKernelGGL(segm_clear_kernel, dim3((unsigned)((nh + ns + NT - 1) / NT)), dim3(NT), 0, st, hist, nh, split, ns);
  const int cblocks = std::min(std::max((HW / 16 + NT * 4 - 1) / (NT * 4), 1), SEGM_MAX_BLOCKS);
  hipLaunchKernelGGL(segm_centroid_kernel, dim3(cblocks, N), dim3(NT), 0, st, gt, H, W, hist, split);
  const int spans = (HW + 3 + SEGM_SPAN - 1) / SEGM_SPAN;
  const int fblocks = std::min(std::max((spans + NT * SEGM_SPANS_PER_LANE - 1) / (NT * SEGM_SPANS_PER_LANE), 1), SEGM_MAX_BLOCKS);
  hipLaunchKernelGGL(segm_fill_kernel, dim3(fblocks, N), dim3(NT), 0, st, pred, (long long)pred_image_stride, gt, H, W, split, hist);
  CK((int)hipGetLastError(), "seg histograms");
  return 0;
}

size_t camo_seg_weighted_f_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (N < 1 || N > CAMO_RGD_MAX_IMAGES || H < 1 || W < 1 || H > CAMO_SEG_WF_MAX_SIDE || W > CAMO_SEG_WF_MAX_SIDE || (long long)H * W < 2) return 0;
  return wf_carve(N, H, W, nullptr).bytes;
}

int camo_seg_weighted_f(const float* pred, int64_t pred_image_stride, const uint8_t* gt, int32_t N, int32_t H, int32_t W,
                        const double* gauss, void* ws, size_t ws_bytes, int64_t* sums, void* stream) {
  if (int e = segm_check(pred, pred_image_stride, gt, N, H, W)) return e;
  if (H > CAMO_SEG_WF_MAX_SIDE || W > CAMO_SEG_WF_MAX_SIDE) return fail(CAMO_E_ARG, "H and W must be at most CAMO_SEG_WF_MAX_SIDE");
  if (!gauss || !ws || !sums) return fail(CAMO_E_ARG, "null pointer argument");
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(CAMO_E_ARG, "the workspace must be 256-byte aligned");
  if ((reinterpret_cast<uintptr_t>(gauss) & 7) || (reinterpret_cast<uintptr_t>(sums) & 7)) return fail(CAMO_E_ARG, "gauss and sums must be 8-byte aligned");
  const WfWs w = wf_carve(N, H, W, ws);
  if (ws_bytes < w.bytes) return fail(CAMO_E_ARG, "workspace smaller than camo_seg_weighted_f_workspace_bytes(N, H, W)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(segm_clear_kernel, dim3((3 * N * 2 + NT - 1) / NT), dim3(NT), 0, st, reinterpret_cast<int*>(sums), 6ll * N,
                     static_cast<int*>(nullptr), 0ll);
  hipLaunchKernelGGL(segm_wf_column_kernel, dim3((W + NT - 1) / NT, N), dim3(NT), 0, st, gt, H, W, w.d2);
  hipLaunchKernelGGL(segm_wf_row_kernel, dim3(H, N), dim3(NT), 0, st, pred, (long long)pred_image_stride, H, W, w.d2, w.src);
  hipLaunchKernelGGL(segm_wf_weight_kernel, dim3((W + SEGM_WF_TILE_X - 1) / SEGM_WF_TILE_X, (H + SEGM_WF_TILE_Y - 1) / SEGM_WF_TILE_Y, N), dim3(NT),
                     0, st, pred, (long long)pred_image_stride, gt, H, W, gauss, w.d2, w.src, reinterpret_cast<unsigned long long*>(sums));
  CK((int)hipGetLastError(), "seg weighted f");
  return 0;
}

}  // extern "C"
