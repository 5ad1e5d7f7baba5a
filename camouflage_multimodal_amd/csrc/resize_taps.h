// The per-axis taps of include/camo_resize.h and the fetch of an interleaved 8-bit pixel, as device code: shared by resize.hip and by
// guided.hip's camo_guided_apply, which samples coefficient planes with camo_resize's bilinear rule.  Integer arithmetic only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/camo_resize.h"

namespace rsz {

typedef long long i64;

// Is off + (H - 1) rs + (W - 1) ps + (C - 1) cs, the largest element index of a footprint, below `elems`?  Every term is >= 0 here; a sum or
// a product that leaves int64 is not.
__device__ __forceinline__ bool footprint_inside(i64 off, i64 H, i64 W, i64 rs, i64 ps, i64 cs, int C, i64 elems) {
  i64 a, b, c, s;
  if (__builtin_mul_overflow(H - 1, rs, &a) || __builtin_mul_overflow(W - 1, ps, &b) || __builtin_mul_overflow((i64)(C - 1), cs, &c)) return false;
  if (__builtin_add_overflow(off, a, &s) || __builtin_add_overflow(s, b, &s) || __builtin_add_overflow(s, c, &s)) return false;
  return s < elems;
}
__device__ __forceinline__ bool side_ok(i64 v) { return v >= 1 && v <= CAMO_RSZ_MAX_SIDE; }

// One axis of one destination pixel: `n` taps i0 .. i0 + n - 1 (crop coordinates; clamped to the crop for the two-tap rule) and their total T.
struct Axis {
  int c0, cs, D, n, i0, w0, w1, lo, hi, T;
  bool area;
};

template <int FILTER>
__device__ __forceinline__ Axis make_axis(int c0, int cs, int D, int d, bool flip) {
  const int dd = flip ? D - 1 - d : d;
  Axis a;
  a.c0 = c0; a.cs = cs; a.D = D; a.area = false; a.lo = a.hi = 0; a.w0 = 1; a.w1 = 0;
  if (FILTER == CAMO_RSZ_NEAREST) {
    a.n = 1; a.T = 1;
    a.i0 = (2 * dd + 1) * cs / (2 * D);                    // (2 dd + 1) cs < 2^14 * 2^13: int32 holds it
  } else if (FILTER == CAMO_RSZ_AREA && cs > D) {
    a.area = true; a.T = cs;
    a.lo = dd * cs; a.hi = a.lo + cs;                        // the destination pixel's interval, in units of 1 / D source pixels
    a.i0 = a.lo / D;
    a.n = (a.hi + D - 1) / D - a.i0;
  } else {
    const int m = (2 * dd + 1) * cs - D;                     // > -D: its floor quotient by 2 D is -1 or the truncated one
    a.n = 2; a.T = 2 * D;
    a.i0 = m < 0 ? -1 : m / (2 * D);
    a.w1 = m - a.i0 * 2 * D;
    a.w0 = 2 * D - a.w1;
  }
  return a;
}

__device__ __forceinline__ void tap(const Axis& a, int k, int& idx, int& w) {
  const int j = a.i0 + k;
  if (a.area) {
    w = min(a.hi, (j + 1) * a.D) - max(a.lo, j * a.D);       // positive for every j of [i0, i0 + n)
    idx = a.c0 + j;
  } else {
    w = k ? a.w1 : a.w0;
    idx = a.c0 + min(max(j, 0), a.cs - 1);
  }
}

// The C bytes of a u8 pixel.  Interleaved channels (ch_stride 1, C >= 2) come as ONE unaligned 4-byte load where those four bytes lie
// inside the buffer -- a third of the load instructions of a packed RGB image, which is what the kernel's time goes by -- and byte by
// byte otherwise.
__device__ __forceinline__ void load_bytes(const uint8_t* __restrict__ pp, i64 room, i64 chs, int C, int (&v)[CAMO_RSZ_MAX_CHANNELS]) {
  if (chs == 1 && C >= 2 && room >= 4) {
    uint32_t q;
    __builtin_memcpy(&q, pp, 4);
    v[0] = q & 255; v[1] = (q >> 8) & 255; v[2] = (q >> 16) & 255; v[3] = q >> 24;
  } else {
#pragma unroll
    for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) v[c] = c < C ? (int)pp[c * chs] : 0;
  }
}

}  // namespace rsz
