// Resampling between ragged native sizes and the fixed working size (include/camo_resize.h): ONE launch over a table of
// strided source and destination footprints, nearest / bilinear / area, u8 or fp32 on either side.  The header's text is the
// definition; everything here is integer arithmetic (u8 sources) or a fixed order of exact double products (fp32 sources), so the
// output is a function of the inputs alone.  The table lives on the device, so the kernel itself checks every row before it touches
// memory: a wrong table can neither read nor write outside the two buffers.
#include "../../include/camo_resize.h"
#include "abi_util.h"
#include "common.h"
#include "resize_taps.h"

namespace {

constexpr int RSZ_NT = 256;      // threads per block; thread t takes pixels t, t + 256, ... of the block's span in row-major order: a wave runs along a row
constexpr int RSZ_PIX = 4;       // destination pixels per thread: one pixel a thread left the launch bound by its blocks' start-up (the table, then
                                 // the taps, then the store, one memory round trip after the other): 128 maps up to ~1000 x 750 took 1.21 ms
// the footprint test, the per-axis taps and the fetch of an interleaved u8 pixel: resize_taps.h, shared with guided.hip
using rsz::i64;
using rsz::footprint_inside;
using rsz::side_ok;
using rsz::Axis;
using rsz::make_axis;
using rsz::tap;
using rsz::load_bytes;

// A pixel's channels to the destination.  Interleaved channels (ch_stride 1) are written from constants, so that the three floats of a
// packed RGB pixel leave as one 12-byte store.
template <typename T>
__device__ __forceinline__ void store_pixel(T* __restrict__ dst, i64 at, i64 chs, int C, const T (&v)[CAMO_RSZ_MAX_CHANNELS]) {
  if (chs == 1 && C == 3) {
    dst[at] = v[0]; dst[at + 1] = v[1]; dst[at + 2] = v[2];
  } else if (chs == 1 && C == 4) {
    dst[at] = v[0]; dst[at + 1] = v[1]; dst[at + 2] = v[2]; dst[at + 3] = v[3];
  } else {
#pragma unroll
    for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c)
      if (c < C) dst[at + c * chs] = v[c];
  }
}

// The fields of a good row, as the pixels use them.
struct Geo {
  i64 s_rs, s_ps, s_cs, d_off, d_rs, d_ps, d_cs;
  int c_y0, c_x0, c_h, c_w, flip, DH, DW;
};

// Destination pixel (y, x) of a good row, all channels.
template <typename S, typename T, int FILTER>
__device__ __forceinline__ void resize_pixel(const S* __restrict__ base, i64 room, T* __restrict__ dst, const Geo& g, int C, int y, int x, bool live) {
  const Axis ay = make_axis<FILTER>(g.c_y0, g.c_h, g.DH, y, (g.flip & 2) != 0);
  const Axis ax = make_axis<FILTER>(g.c_x0, g.c_w, g.DW, x, (g.flip & 1) != 0);
  T out[CAMO_RSZ_MAX_CHANNELS];

  if constexpr (sizeof(S) == 1) {
    i64 num[CAMO_RSZ_MAX_CHANNELS] = {0, 0, 0, 0};
    for (int ky = 0; ky < ay.n; ++ky) {
      int sy, wy;
      tap(ay, ky, sy, wy);
      const i64 rowo = sy * g.s_rs;
      int rsum[CAMO_RSZ_MAX_CHANNELS] = {0, 0, 0, 0};         // <= Tx * 255 < 2^22
      for (int kx = 0; kx < ax.n; ++kx) {
        int sx, wx, v[CAMO_RSZ_MAX_CHANNELS];
        tap(ax, kx, sx, wx);
        const i64 o = rowo + sx * g.s_ps;
        load_bytes(base + o, room - o, g.s_cs, C, v);
#pragma unroll
        for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) rsum[c] += wx * v[c];
      }
#pragma unroll
      for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) num[c] += (i64)wy * rsum[c];
    }
    const i64 den = (i64)ay.T * ax.T;                         // <= 2^28; num <= 255 den
#pragma unroll
    for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) {
      if constexpr (sizeof(T) == 4) {
        out[c] = (T)((double)num[c] / (double)(255 * den));
      } else {
        out[c] = FILTER == CAMO_RSZ_NEAREST ? (T)num[c] : (T)((unsigned long long)(2 * num[c] + den) / (unsigned long long)(2 * den));
      }
    }
  } else {
    int sy0, wy0, sx0, wx0;
    tap(ay, 0, sy0, wy0);
    tap(ax, 0, sx0, wx0);
    if (FILTER == CAMO_RSZ_NEAREST) {                         // one tap of weight 1 over a total of 1: the value itself
#pragma unroll
      for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) out[c] = c < C ? (T)base[sy0 * g.s_rs + sx0 * g.s_ps + c * g.s_cs] : T(0);
    } else {
      int sy1, wy1, sx1, wx1;
      tap(ay, 1, sy1, wy1);
      tap(ax, 1, sx1, wx1);
      const double w00 = (double)(wy0 * wx0), w01 = (double)(wy0 * wx1), w10 = (double)(wy1 * wx0), w11 = (double)(wy1 * wx1);
      const double den = (double)((i64)ay.T * ax.T);
      const S* __restrict__ r0 = base + sy0 * g.s_rs;
      const S* __restrict__ r1 = base + sy1 * g.s_rs;
#pragma unroll
      for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) {
        if (c < C) {
          const i64 co = c * g.s_cs;
          double acc = w00 * (double)r0[sx0 * g.s_ps + co];   // exact products (header): an FMA below rounds as multiply-then-add does
          acc += w01 * (double)r0[sx1 * g.s_ps + co];
          acc += w10 * (double)r1[sx0 * g.s_ps + co];
          acc += w11 * (double)r1[sx1 * g.s_ps + co];
          out[c] = (T)(acc / den);
        } else {
          out[c] = T(0);
        }
      }
    }
  }
  if (live) store_pixel(dst, g.d_off + y * g.d_rs + x * g.d_ps, g.d_cs, C, out);
}

template <typename S, typename T, int FILTER>
__global__ __launch_bounds__(RSZ_NT) void resize_kernel(const S* __restrict__ src, i64 src_elems, T* __restrict__ dst, i64 dst_elems,
                                                        const i64* __restrict__ table, int C, i64 max_dst_pixels, int* __restrict__ status) {
  const int img = blockIdx.y;
  const i64* __restrict__ r = table + (i64)img * CAMO_RSZ_FIELDS;
  const i64 s_off = r[0], s_H = r[1], s_W = r[2], s_rs = r[3], s_ps = r[4], s_cs = r[5];
  const i64 c_y0 = r[6], c_x0 = r[7], c_h = r[8], c_w = r[9], flip = r[10];
  const i64 d_off = r[11], d_H = r[12], d_W = r[13], d_rs = r[14], d_ps = r[15], d_cs = r[16], rsv = r[17];

  // the destination's own fields first: they say which blocks have pixels, also of a row that is refused
  const bool dst_form = d_off >= 0 && side_ok(d_H) && side_ok(d_W) && d_rs >= 1 && d_ps >= 1 && d_cs >= 1 && d_H * d_W <= max_dst_pixels;
  bool ok = dst_form && s_off >= 0 && side_ok(s_H) && side_ok(s_W) && side_ok(c_h) && side_ok(c_w) && s_rs >= 1 && s_ps >= 1 && s_cs >= 1 &&
            c_y0 >= 0 && c_x0 >= 0 && c_y0 <= s_H - c_h && c_x0 <= s_W - c_w && flip >= 0 && flip <= 3 && rsv == 0;
  ok = ok && footprint_inside(s_off, s_H, s_W, s_rs, s_ps, s_cs, C, src_elems) && footprint_inside(d_off, d_H, d_W, d_rs, d_ps, d_cs, C, dst_elems);
  if (threadIdx.x == 0) status[img] = ok ? 0 : 1;
  if (!dst_form) return;
  const int DH = (int)d_H, DW = (int)d_W, npix = DH * DW;
  const int first = blockIdx.x * (RSZ_NT * RSZ_PIX) + threadIdx.x;    // < max_dst_pixels + 1024 <= 2^26 + 1024
  if (first - (int)threadIdx.x >= npix) return;

  if (!ok) {                                                  // zeros over the stated destination where it lies inside dst; nothing is read
    for (int k = 0; k < RSZ_PIX; ++k) {
      const int pix = first + k * RSZ_NT;
      if (pix >= npix) return;
      const int y = pix / DW, x = pix - y * DW;
      i64 a, b, at;
      if (__builtin_mul_overflow((i64)y, d_rs, &a) || __builtin_mul_overflow((i64)x, d_ps, &b) || __builtin_add_overflow(d_off, a, &at) ||
          __builtin_add_overflow(at, b, &at))
        continue;
      for (int c = 0; c < C; ++c) {
        i64 e;
        if (__builtin_mul_overflow((i64)c, d_cs, &e) || __builtin_add_overflow(at, e, &e)) break;
        if (e < dst_elems) dst[e] = T(0);
      }
    }
    return;
  }

  const Geo g = {s_rs, s_ps, s_cs, d_off, d_rs, d_ps, d_cs, (int)c_y0, (int)c_x0, (int)c_h, (int)c_w, (int)flip, DH, DW};
#pragma unroll
  for (int k = 0; k < RSZ_PIX; ++k) {                         // independent pixels with no branch between them: their loads are in flight together
    const int at = first + k * RSZ_NT, pix = min(at, npix - 1);  // (past the image: the last pixel once more, and no store)
    const int y = pix / DW;
    resize_pixel<S, T, FILTER>(src + s_off, src_elems - s_off, dst, g, C, y, pix - y * DW, at < npix);
  }
}

template <typename S, typename T>
int launch_filter(int filter, dim3 grid, hipStream_t st, const void* src, i64 src_elems, void* dst, i64 dst_elems, const i64* table, int C,
                  i64 max_dst_pixels, int* status) {
  const S* s = static_cast<const S*>(src);
  T* d = static_cast<T*>(dst);
  if (filter == CAMO_RSZ_NEAREST)
    hipLaunchKernelGGL((resize_kernel<S, T, CAMO_RSZ_NEAREST>), grid, dim3(RSZ_NT), 0, st, s, src_elems, d, dst_elems, table, C, max_dst_pixels, status);
  else if (filter == CAMO_RSZ_BILINEAR)
    hipLaunchKernelGGL((resize_kernel<S, T, CAMO_RSZ_BILINEAR>), grid, dim3(RSZ_NT), 0, st, s, src_elems, d, dst_elems, table, C, max_dst_pixels, status);
  else if constexpr (sizeof(S) == 1)
    hipLaunchKernelGGL((resize_kernel<S, T, CAMO_RSZ_AREA>), grid, dim3(RSZ_NT), 0, st, s, src_elems, d, dst_elems, table, C, max_dst_pixels, status);
  return (int)hipGetLastError();
}

}  // namespace

using camo_abi::fail;

extern "C" int camo_resize(const void* src, int64_t src_elems, int32_t src_type, void* dst, int64_t dst_elems, int32_t dst_type,
                           const int64_t* table, int32_t N, int32_t C, int32_t filter, int64_t max_dst_pixels, int32_t* status, void* stream) {
  if (!src) return fail(CAMO_E_ARG, "src is null");
  if (!dst) return fail(CAMO_E_ARG, "dst is null");
  if (!table) return fail(CAMO_E_ARG, "table is null");
  if (!status) return fail(CAMO_E_ARG, "status is null");
  if (N < 1 || N > CAMO_RGD_MAX_IMAGES) return fail(CAMO_E_ARG, "need 1 <= N <= CAMO_RGD_MAX_IMAGES");
  if (C < 1 || C > CAMO_RSZ_MAX_CHANNELS) return fail(CAMO_E_ARG, "need 1 <= C <= CAMO_RSZ_MAX_CHANNELS");
  if (filter != CAMO_RSZ_NEAREST && filter != CAMO_RSZ_BILINEAR && filter != CAMO_RSZ_AREA) return fail(CAMO_E_ARG, "filter is none of CAMO_RSZ_NEAREST, _BILINEAR, _AREA");
  if (src_type != CAMO_RSZ_U8 && src_type != CAMO_RSZ_F32) return fail(CAMO_E_ARG, "src_type is neither CAMO_RSZ_U8 nor CAMO_RSZ_F32");
  if (dst_type != CAMO_RSZ_U8 && dst_type != CAMO_RSZ_F32) return fail(CAMO_E_ARG, "dst_type is neither CAMO_RSZ_U8 nor CAMO_RSZ_F32");
  if (src_type == CAMO_RSZ_F32 && dst_type == CAMO_RSZ_U8) return fail(CAMO_E_ARG, "dst_type CAMO_RSZ_U8 takes a CAMO_RSZ_U8 source only (fp32 -> u8 is not defined)");
  if (src_type == CAMO_RSZ_F32 && filter == CAMO_RSZ_AREA) return fail(CAMO_E_ARG, "filter CAMO_RSZ_AREA takes a CAMO_RSZ_U8 source only");
  if (max_dst_pixels < 1 || max_dst_pixels > (int64_t)CAMO_RSZ_MAX_SIDE * CAMO_RSZ_MAX_SIDE) return fail(CAMO_E_ARG, "need 1 <= max_dst_pixels <= CAMO_RSZ_MAX_SIDE^2");
  if (src_elems < 1) return fail(CAMO_E_ARG, "need src_elems >= 1");
  if (dst_elems < 1) return fail(CAMO_E_ARG, "need dst_elems >= 1");
  if (src_type == CAMO_RSZ_F32 && (reinterpret_cast<uintptr_t>(src) & 3)) return fail(CAMO_E_ARG, "an fp32 src must be 4-byte aligned");
  if (dst_type == CAMO_RSZ_F32 && (reinterpret_cast<uintptr_t>(dst) & 3)) return fail(CAMO_E_ARG, "an fp32 dst must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(CAMO_E_ARG, "table must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(status) & 3) return fail(CAMO_E_ARG, "status must be 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((max_dst_pixels + RSZ_NT * RSZ_PIX - 1) / (RSZ_NT * RSZ_PIX)), (unsigned)N);
  const i64* tb = reinterpret_cast<const i64*>(table);
  int e;
  if (src_type == CAMO_RSZ_F32)
    e = launch_filter<float, float>(filter, grid, st, src, src_elems, dst, dst_elems, tb, C, max_dst_pixels, status);
  else if (dst_type == CAMO_RSZ_F32)
    e = launch_filter<uint8_t, float>(filter, grid, st, src, src_elems, dst, dst_elems, tb, C, max_dst_pixels, status);
  else
    e = launch_filter<uint8_t, uint8_t>(filter, grid, st, src, src_elems, dst, dst_elems, tb, C, max_dst_pixels, status);
  CK(e, "resize");
  return 0;
}
