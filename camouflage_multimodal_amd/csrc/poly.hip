// COCO polygon annotations to label maps (include/camo_poly.h): COCO's rleFrPoly and the union of an annotation's
// polygons, per edge and per word instead of point by point.  Every grid covers the whole call; FOUR launches whatever N, A, P and V.
//
//   verdict  one wave per polygon: step 7 of the header into poly_ok; the blocks past the polygons clear the label maps and one
//            toggle bit-plane per polygon (a bit per position p = x H + y)
//   toggle   one wave per edge, lanes over the edge's boundary points in strides of 64: a lane takes its point from the closed form
//            and the point before it from the lane below (lane 0: the closed form again, or the last point of the edge before);
//            one 32-bit atomicXor per toggle.  The blocks past the edges take the verdict of every annotation (a wave each, lanes
//            over its polygons) and set ann_area to 0 or -1
//   scan     one block per polygon: inclusive prefix-XOR of the plane, four words a thread (five shift-XORs inside a word, the
//            carry into a word is the parity of the popcounts before it: within the thread, a ballot of the lanes' parities, the
//            waves' through LDS, and one bit from pass to pass).  The plane then holds the mask in position order
//   paint    one thread per (annotation, word): OR of the annotation's planes, popcount into one 64-bit atomicAdd a wave, one
//            32-bit atomicMax per set bit at (p % H, p / H)
//
// The only floating point is the header's: one multiply and one add per vertex coordinate, one division per edge, one multiply and
// two adds per boundary point, each rounded once.  hipcc contracts a * b + c into a fused multiply-add by default, and its
// __dmul_rn / __dadd_rn are plain operators that it contracts as well, so contraction is switched OFF for this file: by the pragma
// below for the code written here and by -ffp-contract=off in build.py's EXTRA_FLAGS for whatever is inlined into it.  The only
// v_fma_f64 left in the object are those of the division's own expansion (tests/test_poly.py holds cases that a fused kernel misses).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "common.h"
#include "poly.h"
#include "../../include/camo_poly.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, WAVES = NT / 64;
constexpr int SCAN_ITEMS = 4;            // consecutive words a thread of the scan takes in a pass: one 16-byte load, 1024 words a pass
constexpr int TOGGLE_MAX_Y = 32;         // blocks that share a polygon's edges at the most
constexpr int FLOOR_SHIFT = 1 << 13;     // added in fives to a boundary coordinate (>= -5 CAMO_POLY_MARGIN) before / and %: both floor
static_assert(5 * FLOOR_SHIFT > 5 * CAMO_POLY_MARGIN + 8, "the shifted coordinates are positive");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// step 1: (int)(5.0 * c + 0.5), the product and the sum rounded once each, the conversion toward zero
__device__ __forceinline__ int scaled(double c) {
  const double product = 5.0 * c;
  return (int)(product + 0.5);
}

// (int)(a + s * t + 0.5) of step 2
__device__ __forceinline__ int along(int a, double s, int t) {
  const double product = s * (double)t;
  const double sum = (double)a + product;
  return (int)(sum + 0.5);
}

// One edge after the swap of step 2: n = len + 1 boundary points.
struct Edge {
  int xs, ys, len;
  bool xmajor, flip;
  double s;
};

__device__ __forceinline__ Edge make_edge(int xs, int ys, int xe, int ye) {
  Edge e;
  const int dx = abs(xe - xs), dy = abs(ye - ys);
  e.xmajor = dx >= dy;
  e.flip = e.xmajor ? xs > xe : ys > ye;
  if (e.flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
  e.xs = xs; e.ys = ys;
  e.len = e.xmajor ? dx : dy;
  e.s = e.len > 0 ? (double)(e.xmajor ? ye - ys : xe - xs) / (double)e.len : 0.0;      // (IEEE division: correctly rounded)
  return e;
}

__device__ __forceinline__ int2 edge_point(const Edge& e, int d) {
  if (e.len == 0) return make_int2(e.xs, e.ys);                      // (the one point of an edge of no length)
  const int t = e.flip ? e.len - d : d;
  return e.xmajor ? make_int2(e.xs + t, along(e.ys, e.s, t)) : make_int2(along(e.xs, e.s, t), e.ys + t);
}

// grid (verdict blocks + clear blocks).  Block b < verdict_blocks: poly_ok of polygons b * WAVES + wave, + verdict_blocks * WAVES, ...
__global__ __launch_bounds__(NT) void poly_verdict_kernel(const double* __restrict__ xy, int V, const int* __restrict__ poly_off, int P, int H, int W,
                                                          int verdict_blocks, int* __restrict__ poly_ok, int* __restrict__ labels, long long pixels,
                                                          uint4* __restrict__ planes, long long plane_quads) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= verdict_blocks) {                           // (the whole block)
    const long long step = (long long)(gridDim.x - verdict_blocks) * NT, first = (long long)(blockIdx.x - verdict_blocks) * NT + tid;
    for (long long i = first; i < pixels; i += step) labels[i] = 0;
    for (long long i = first; i < plane_quads; i += step) planes[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const double x_lo = -(double)CAMO_POLY_MARGIN, x_hi = (double)W + CAMO_POLY_MARGIN, y_hi = (double)H + CAMO_POLY_MARGIN;
  for (int p = blockIdx.x * WAVES + wave; p < P; p += verdict_blocks * WAVES) {
    const int lo = clampi(poly_off[p], 0, V), hi = clampi(poly_off[p + 1], lo, V);      // (inside xy whatever poly_off holds)
    bool bad = hi == lo;
    for (int i = lo + lane; i < hi; i += 64) {
      const double x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
      bad |= !(x >= x_lo && x <= x_hi && y >= x_lo && y <= y_hi);    // (a NaN fails every comparison)
    }
    const bool any_bad = __any(bad);
    if (lane == 0) poly_ok[p] = any_bad ? 0 : 1;
  }
}

// grid (P * EY + annotation blocks).  Block b < P * EY: the edges (b % EY) * WAVES + wave, + EY * WAVES, ... of polygon b / EY.
__global__ __launch_bounds__(NT) void poly_toggle_kernel(const double* __restrict__ xy, int V, const int* __restrict__ poly_off, int P, int EY,
                                                         const int* __restrict__ poly_ok, int H, int W, unsigned* __restrict__ planes, size_t stride,
                                                         const int* __restrict__ ann_poly_off, const int* __restrict__ ann_image,
                                                         const int* __restrict__ ann_value, int A, int N, int* __restrict__ ann_ok,
                                                         long long* __restrict__ ann_area) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int edge_blocks = P * EY;
  if ((int)blockIdx.x >= edge_blocks) {                              // (the whole block): the annotations' verdicts
    const int blocks = gridDim.x - edge_blocks;
    for (int a = (blockIdx.x - edge_blocks) * WAVES + wave; a < A; a += blocks * WAVES) {
      const int lo = clampi(ann_poly_off[a], 0, P), hi = clampi(ann_poly_off[a + 1], lo, P);      // (inside poly_ok whatever it holds)
      bool bad = false;
      for (int q = lo + lane; q < hi; q += 64) bad |= poly_ok[q] == 0;
      const bool ok = !__any(bad) && ann_image[a] >= 0 && ann_image[a] < N && ann_value[a] >= 1;
      if (lane == 0) { ann_ok[a] = ok ? 1 : 0; ann_area[a] = ok ? 0 : -1; }
    }
    return;
  }
  const int p = blockIdx.x / EY, part = blockIdx.x - p * EY;
  if (!poly_ok[p]) return;                                           // (so lo < hi and every coordinate converts)
  const int lo = clampi(poly_off[p], 0, V), hi = clampi(poly_off[p + 1], lo, V), k = hi - lo;
  unsigned* plane = planes + (size_t)p * stride;
  const int HW = H * W;
  for (int j = part * WAVES + wave; j < k; j += EY * WAVES) {        // (wave-uniform)
    const double* a = xy + 2 * (size_t)(lo + j);
    const double* b = xy + 2 * (size_t)(lo + (j + 1 == k ? 0 : j + 1));
    const int xa = scaled(a[0]), ya = scaled(a[1]);
    const Edge e = make_edge(xa, ya, scaled(b[0]), scaled(b[1]));
    int2 before = make_int2(0, 0);                                   // the point in front of this edge's first: the last of edge j - 1
    if (j > 0) {
      const double* z = xy + 2 * (size_t)(lo + j - 1);
      const Edge prev = make_edge(scaled(z[0]), scaled(z[1]), xa, ya);
      before = edge_point(prev, prev.len);
    }
    for (int d0 = 0; d0 <= e.len; d0 += 64) {                        // (wave-uniform: the shuffle below takes every lane)
      const int d = d0 + lane;
      const bool live = d <= e.len;
      const int2 cur = edge_point(e, live ? d : e.len);
      int2 pre;
      pre.x = __shfl_up(cur.x, 1, 64);
      pre.y = __shfl_up(cur.y, 1, 64);
      if (lane == 0) pre = d0 > 0 ? edge_point(e, d0 - 1) : before;
      if (!live || (d == 0 && j == 0) || cur.x == pre.x) continue;   // the polygon's first point has none before it
      const int m = min(cur.x, pre.x) + 5 * FLOOR_SHIFT;             // step 3, in integers
      if (m % 5 != 2) continue;
      const int x = m / 5 - FLOOR_SHIFT;
      if (x < 0 || x > W - 1) continue;
      const int y = clampi((min(cur.y, pre.y) + 2 + 5 * FLOOR_SHIFT) / 5 - FLOOR_SHIFT, 0, H);      // ceil((v - 2) / 5) = floor((v + 2) / 5)
      const int pos = x * H + y;
      if (pos < HW) atomicXor(plane + (pos >> 5), 1u << (pos & 31));
    }
  }
}

__device__ __forceinline__ unsigned prefix_xor(unsigned x) {
  x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
  return x;
}

// grid (max(P, 1)): the plane of polygon blockIdx.x from toggles to mask
__global__ __launch_bounds__(NT) void poly_scan_kernel(const int* __restrict__ poly_ok, int P, unsigned* __restrict__ planes, size_t stride) {
  __shared__ unsigned wpar[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = blockIdx.x;
  if (p >= P || !poly_ok[p]) return;                                 // (the whole block; the plane of a polygon that is not ok stays clear)
  uint4* plane = reinterpret_cast<uint4*>(planes + (size_t)p * stride);
  const size_t quads = stride / SCAN_ITEMS;
  unsigned carry = 0;                                                // parity of every toggle before this pass
  for (size_t q0 = 0; q0 < quads; q0 += NT) {                        // (block-uniform)
    const size_t q = q0 + tid;
    uint4 v = q < quads ? plane[q] : make_uint4(0u, 0u, 0u, 0u);
    unsigned w[SCAN_ITEMS] = {v.x, v.y, v.z, v.w}, mine = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
      const unsigned x = prefix_xor(w[i]);
      w[i] = mine ? ~x : x;
      mine ^= x >> 31;                                               // (the word's own parity)
    }
    const unsigned long long votes = __ballot(mine != 0);
    if (lane == 0) wpar[wave] = __popcll(votes) & 1;
    __syncthreads();
    unsigned in = carry ^ (__popcll(votes & ((1ull << lane) - 1ull)) & 1);
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
      if (i < wave) in ^= wpar[i];
      carry ^= wpar[i];
    }
    if (q < quads) plane[q] = in ? make_uint4(~w[0], ~w[1], ~w[2], ~w[3]) : make_uint4(w[0], w[1], w[2], w[3]);
    __syncthreads();
  }
}

// grid (word blocks, annotation rows): annotations blockIdx.y, + gridDim.y, ...; words blockIdx.x * NT + tid, + gridDim.x * NT, ...
__global__ __launch_bounds__(NT) void poly_paint_kernel(const unsigned* __restrict__ planes, size_t stride, int P, const int* __restrict__ ann_poly_off,
                                                        const int* __restrict__ ann_image, const int* __restrict__ ann_value,
                                                        const int* __restrict__ ann_ok, int A, int H, int W, int* __restrict__ labels,
                                                        long long* __restrict__ ann_area) {
  const int lane = threadIdx.x & 63;
  const int HW = H * W, words = (HW + 31) >> 5;
  for (int a = blockIdx.y; a < A; a += gridDim.y) {                  // (block-uniform)
    if (!ann_ok[a]) continue;                                        // (so its image and value are in range and its polygons ok)
    const int lo = clampi(ann_poly_off[a], 0, P), hi = clampi(ann_poly_off[a + 1], lo, P);
    int* img = labels + (size_t)ann_image[a] * HW;
    const int value = ann_value[a];
    long long area = 0;
    for (int w = blockIdx.x * NT + threadIdx.x; w < words; w += gridDim.x * NT) {
      unsigned m = 0;
      for (int q = lo; q < hi; ++q) m |= planes[(size_t)q * stride + w];
      if (w == words - 1 && (HW & 31)) m &= (1u << (HW & 31)) - 1u;    // the scan runs on past the last position
      area += __popc(m);
      while (m) {
        const int pos = w * 32 + __ffs(m) - 1;
        m &= m - 1;
        const int x = pos / H, y = pos - x * H;
        atomicMax(img + (size_t)y * W + x, value);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) area += __shfl_xor(area, o, 64);
    if (lane == 0 && area > 0) atomicAdd(reinterpret_cast<unsigned long long*>(ann_area + a), (unsigned long long)area);
  }
}

}  // namespace

PolyWs poly_carve(int H, int W, int A, int P, void* base) {
  PolyWs w{};
  camo_abi::Carver c(base);
  w.stride = (((size_t)H * W + 31) / 32 + SCAN_ITEMS - 1) / SCAN_ITEMS * SCAN_ITEMS;
  w.plane = c.take<unsigned>(std::max<size_t>((size_t)P * w.stride, 1));
  w.poly_ok = c.take<int>((size_t)std::max(P, 1));
  w.ann_ok = c.take<int>((size_t)std::max(A, 1));
  w.bytes = c.bytes();
  return w;
}

int launch_poly_decode(const double* xy, int V, const int* poly_off, int P, const int* ann_poly_off, const int* ann_image, const int* ann_value,
                       int A, int N, int H, int W, const PolyWs& ws, int* labels, long long* ann_area, hipStream_t stream) {
  const long long pixels = (long long)N * H * W, plane_quads = (long long)P * (long long)(ws.stride / SCAN_ITEMS);
  const int verdict_blocks = std::min((P + WAVES - 1) / WAVES, 1024);
  const unsigned clear_blocks = (unsigned)std::min<long long>((std::max(pixels, plane_quads) + NT - 1) / NT, 4096);
  hipLaunchKernelGGL(poly_verdict_kernel, dim3(verdict_blocks + clear_blocks), dim3(NT), 0, stream, xy, V, poly_off, P, H, W, verdict_blocks, ws.poly_ok,
                     labels, pixels, reinterpret_cast<uint4*>(ws.plane), plane_quads);
  // the blocks that share a polygon: about one wave an edge of the mean polygon
  const int EY = P > 0 ? (int)std::min<long long>(std::max<long long>(((long long)V / P + WAVES - 1) / WAVES, 1), TOGGLE_MAX_Y) : 0;
  const int ann_blocks = std::min((A + WAVES - 1) / WAVES, 1024);
  hipLaunchKernelGGL(poly_toggle_kernel, dim3((unsigned)(P * EY + ann_blocks)), dim3(NT), 0, stream, xy, V, poly_off, P, EY, ws.poly_ok, H, W, ws.plane,
                     ws.stride, ann_poly_off, ann_image, ann_value, A, N, ws.ann_ok, ann_area);
  hipLaunchKernelGGL(poly_scan_kernel, dim3((unsigned)std::max(P, 1)), dim3(NT), 0, stream, ws.poly_ok, P, ws.plane, ws.stride);
  const int words = (H * W + 31) / 32;
  const dim3 paint((unsigned)std::min((words + NT - 1) / NT, 1024), (unsigned)std::min(A, 65535));
  hipLaunchKernelGGL(poly_paint_kernel, paint, dim3(NT), 0, stream, ws.plane, ws.stride, P, ann_poly_off, ann_image, ann_value, ws.ann_ok, A, H, W, labels,
                     ann_area);
  return (int)hipGetLastError();
}
