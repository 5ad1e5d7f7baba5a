// The training augmentation (include/camo_augment.h): packed uint8 sources of mixed sizes through one inverse affine map per
// image into a dense batch, then -- optionally -- PIL's four ImageEnhance operations restated in integers.  The header's text is the
// definition; everything here is integer arithmetic and the one accumulation across blocks is a 64-bit integer atomic, so the output is a
// function of the inputs alone.  The table lives on the device, so the kernels themselves check every row before they touch memory.
#include "../../include/camo_augment.h"
#include "abi_util.h"
#include "common.h"
#include "resize_taps.h"

namespace {

constexpr int AUG_NT = 256;      // threads per block, both kernels
constexpr int AUG_PIX = 4;       // destination pixels per thread (resize.hip's geometry: pixels t, t + 256, ... of the block's span, a wave along a row)
constexpr int AUG_F = CAMO_AUG_FRAC_BITS;
constexpr int AUG_TILE = CAMO_AUG_TILE;
constexpr int AUG_HALO = AUG_TILE + 2;
using rsz::i64;
using rsz::footprint_inside;
using rsz::side_ok;
using rsz::load_bytes;
typedef unsigned long long u64;

// blend(deg, v, k) of the header: |deg (256 - k) + v k + 128| < 2^19, and >> of a negative int is the floor
__device__ __forceinline__ int blend(int deg, int v, int k) { return min(max((deg * (256 - k) + v * k + 128) >> 8, 0), 255); }
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// The header's row conditions.  `r` is the image's row; nothing else is read.
__device__ __forceinline__ bool row_good(const i64* __restrict__ r, int C, i64 src_elems, int enhance) {
  const i64 s_off = r[0], s_H = r[1], s_W = r[2], s_rs = r[3], s_ps = r[4], s_cs = r[5], c_y0 = r[6], c_x0 = r[7], c_h = r[8], c_w = r[9];
  bool ok = s_off >= 0 && side_ok(s_H) && side_ok(s_W) && side_ok(c_h) && side_ok(c_w) && s_rs >= 1 && s_ps >= 1 && s_cs >= 1 && c_y0 >= 0 &&
            c_x0 >= 0 && c_y0 <= s_H - c_h && c_x0 <= s_W - c_w;
  const i64 A = (i64)1 << 30, B = (i64)1 << 46;
  ok = ok && r[10] >= -A && r[10] <= A && r[11] >= -A && r[11] <= A && r[13] >= -A && r[13] <= A && r[14] >= -A && r[14] <= A;
  ok = ok && r[12] >= -B && r[12] <= B && r[15] >= -B && r[15] <= B;
  ok = ok && (r[16] == 0 || r[16] == 1) && r[17] >= 0 && r[17] < ((i64)1 << 32) && r[22] == 0 && r[23] == 0;
  if (enhance)
    ok = ok && r[18] >= 0 && r[18] <= CAMO_AUG_MAX_FACTOR && r[19] >= 0 && r[19] <= CAMO_AUG_MAX_FACTOR && r[20] >= 0 && r[20] <= CAMO_AUG_MAX_FACTOR &&
         r[21] >= 0 && r[21] <= CAMO_AUG_MAX_FACTOR;
  return ok && footprint_inside(s_off, s_H, s_W, s_rs, s_ps, s_cs, C, src_elems);
}

// The fields of a good row, as the pixels use them.
struct Map {
  i64 s_rs, s_ps, s_cs, a00, a01, b0, a10, a11, b1;
  int y_lo, y_hi, x_lo, x_hi;      // the clip box, both ends inside
  unsigned fill;
  bool constant;
};

// One tap: the source pixel at (iy, ix) clamped into the clip box -- always inside the source, so the load is unconditional -- and the fill
// bytes in its place where the tap lies outside the box and the border is constant.
__device__ __forceinline__ void tap_pixel(const uint8_t* __restrict__ base, i64 room, const Map& m, int C, i64 iy, i64 ix, int (&v)[CAMO_RSZ_MAX_CHANNELS]) {
  const int cy = (int)min(max(iy, (i64)m.y_lo), (i64)m.y_hi), cx = (int)min(max(ix, (i64)m.x_lo), (i64)m.x_hi);
  const i64 o = cy * m.s_rs + cx * m.s_ps;
  load_bytes(base + o, room - o, m.s_cs, C, v);
  if (m.constant && (cy != iy || cx != ix)) {
#pragma unroll
    for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) v[c] = (m.fill >> (8 * c)) & 255;
  }
}

// Destination pixel (y, x) of a good row: num of the header per channel, over den = 1 (NEAREST) or 2^32 (BILINEAR).
template <int FILTER>
__device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ base, i64 room, const Map& m, int C, int y, int x, i64 (&num)[CAMO_RSZ_MAX_CHANNELS]) {
  const i64 X = m.a00 * (2 * x + 1) + m.a01 * (2 * y + 1) + m.b0;      // |X|, |Y| < 2^47 (header)
  const i64 Y = m.a10 * (2 * x + 1) + m.a11 * (2 * y + 1) + m.b1;
  if (FILTER == CAMO_RSZ_NEAREST) {
    int v[CAMO_RSZ_MAX_CHANNELS];
    tap_pixel(base, room, m, C, (Y + (1 << (AUG_F - 1))) >> AUG_F, (X + (1 << (AUG_F - 1))) >> AUG_F, v);
#pragma unroll
    for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) num[c] = v[c];
  } else {
    const i64 ix = X >> AUG_F, iy = Y >> AUG_F;                         // >> of a negative int64 is the floor
    const int wx1 = (int)(X & ((1 << AUG_F) - 1)), wx0 = (1 << AUG_F) - wx1, wy1 = (int)(Y & ((1 << AUG_F) - 1)), wy0 = (1 << AUG_F) - wy1;
    int p00[CAMO_RSZ_MAX_CHANNELS], p01[CAMO_RSZ_MAX_CHANNELS], p10[CAMO_RSZ_MAX_CHANNELS], p11[CAMO_RSZ_MAX_CHANNELS];
    tap_pixel(base, room, m, C, iy, ix, p00);
    tap_pixel(base, room, m, C, iy, ix + 1, p01);
    tap_pixel(base, room, m, C, iy + 1, ix, p10);
    tap_pixel(base, room, m, C, iy + 1, ix + 1, p11);
#pragma unroll
    for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c)                     // a row's sum <= 255 2^16
      num[c] = (i64)wy0 * (wx0 * p00[c] + wx1 * p01[c]) + (i64)wy1 * (wx0 * p10[c] + wx1 * p11[c]);
  }
}

template <int FILTER>
__device__ __forceinline__ int to_u8(i64 num) { return FILTER == CAMO_RSZ_NEAREST ? (int)num : (int)((num + ((i64)1 << 31)) >> 32); }

__global__ __launch_bounds__(AUG_NT) void aug_clear_kernel(u64* __restrict__ sums, int N) {
  const int i = blockIdx.x * AUG_NT + threadIdx.x;
  if (i < N) sums[i] = 0;
}

// enhance = 0: T is dst's type and the pixels go to dst.  ENH: T is uint32_t, dst is the staging image in ws (one word per pixel: R, G, B
// after brightness in bytes 0, 1, 2), C is 3 and the block's luma sum goes to sums[img].
template <typename T, int FILTER, bool ENH>
__global__ __launch_bounds__(AUG_NT) void aug_warp_kernel(const uint8_t* __restrict__ src, i64 src_elems, T* __restrict__ dst, const i64* __restrict__ table,
                                                          int C, int Ho, int Wo, int* __restrict__ status, u64* __restrict__ sums) {
  const int img = blockIdx.y;
  const i64* __restrict__ r = table + (i64)img * CAMO_AUG_FIELDS;
  const bool ok = row_good(r, C, src_elems, ENH ? 1 : 0);
  if (threadIdx.x == 0) status[img] = ok ? 0 : 1;
  const int npix = Ho * Wo;                                             // <= 2^26
  const int first = blockIdx.x * (AUG_NT * AUG_PIX) + threadIdx.x;
  const int W = ENH ? 1 : C;                                            // elements of T per pixel
  T* __restrict__ out = dst + (i64)img * npix * W;
  if (!ok) {                                                            // nothing is read; the enhancement kernel stores the zeros of a staged row
    if (!ENH) {
      for (int k = 0; k < AUG_PIX; ++k) {
        const int pix = first + k * AUG_NT;
        if (pix >= npix) break;
        for (int c = 0; c < C; ++c) out[(i64)pix * C + c] = T(0);
      }
    }
    return;
  }
  const Map m = {r[3], r[4], r[5], r[10], r[11], r[12], r[13], r[14], r[15], (int)r[6], (int)(r[6] + r[8] - 1), (int)r[7], (int)(r[7] + r[9] - 1),
                 (unsigned)r[17], r[16] == 0};
  const int kb = ENH ? (int)r[18] : 256;
  const uint8_t* __restrict__ base = src + r[0];
  const i64 room = src_elems - r[0];
  int lsum = 0;
#pragma unroll
  for (int k = 0; k < AUG_PIX; ++k) {                                   // independent pixels: their loads are in flight together
    const int at = first + k * AUG_NT, pix = min(at, npix - 1);         // (past the image: the last pixel once more, and no store)
    const int y = pix / Wo;
    i64 num[CAMO_RSZ_MAX_CHANNELS];
    warp_pixel<FILTER>(base, room, m, C, y, pix - y * Wo, num);
    if constexpr (ENH) {
      const int R = blend(0, to_u8<FILTER>(num[0]), kb), G = blend(0, to_u8<FILTER>(num[1]), kb), B = blend(0, to_u8<FILTER>(num[2]), kb);
      if (at < npix) {
        out[pix] = (T)(R | (G << 8) | (B << 16));
        lsum += luma(R, G, B);
      }
    } else if (at < npix) {
      T v[CAMO_RSZ_MAX_CHANNELS];
#pragma unroll
      for (int c = 0; c < CAMO_RSZ_MAX_CHANNELS; ++c) {
        if constexpr (sizeof(T) == 4)
          v[c] = (T)((double)num[c] / (FILTER == CAMO_RSZ_NEAREST ? 255.0 : 255.0 * 4294967296.0));
        else
          v[c] = (T)to_u8<FILTER>(num[c]);
      }
      const i64 o = (i64)pix * C;
      if (C == 3) {
        out[o] = v[0]; out[o + 1] = v[1]; out[o + 2] = v[2];
      } else if (C == 4) {
        out[o] = v[0]; out[o + 1] = v[1]; out[o + 2] = v[2]; out[o + 3] = v[3];
      } else {
#pragma unroll
        for (int c = 0; c < 2; ++c)
          if (c < C) out[o + c] = v[c];
      }
    }
  }
  if constexpr (ENH) {                                                  // the block's luma sum (<= 1024 * 255): wave, block, ONE integer atomic
    __shared__ int part[AUG_NT / 64];
    for (int d = 32; d >= 1; d >>= 1) lsum += __shfl_down(lsum, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[img], (u64)(part[0] + part[1] + part[2] + part[3]));
  }
}

// Contrast, colour and sharpness of one 32 x 32 tile of the staged image.  Contrast and colour are pointwise, so the halo's pixels are
// recomputed here, not exchanged between blocks; the 3 x 3 sums are taken from LDS.
template <typename T>
__global__ __launch_bounds__(AUG_NT) void aug_enhance_kernel(const uint32_t* __restrict__ staged, const u64* __restrict__ sums, T* __restrict__ dst,
                                                             const i64* __restrict__ table, int Ho, int Wo, int tiles_x, const int* __restrict__ status) {
  __shared__ uint32_t tile[AUG_HALO][AUG_HALO + 1];
  const int img = blockIdx.y, npix = Ho * Wo;
  const int ty0 = (blockIdx.x / tiles_x) * AUG_TILE, tx0 = (blockIdx.x % tiles_x) * AUG_TILE;
  const int lx = threadIdx.x & (AUG_TILE - 1), ly0 = threadIdx.x / AUG_TILE;     // the thread's pixels: column lx, rows ly0, + 8, + 16, + 24 of the tile
  T* __restrict__ out = dst + (i64)img * npix * 3;
  if (status[img] != 0) {                                               // a refused row: zeros, and neither the table's factors nor ws are read
    for (int k = 0; k < AUG_PIX; ++k) {
      const int y = ty0 + ly0 + k * (AUG_NT / AUG_TILE), x = tx0 + lx;
      if (y < Ho && x < Wo) {
        const i64 o = ((i64)y * Wo + x) * 3;
        out[o] = T(0); out[o + 1] = T(0); out[o + 2] = T(0);
      }
    }
    return;
  }
  const i64* __restrict__ r = table + (i64)img * CAMO_AUG_FIELDS;
  const int kc = (int)r[19], ks = (int)r[20], kh = (int)r[21];          // in [0, 1024]: the warp kernel found the row good
  const int mean = (int)((2 * sums[img] + (u64)npix) / (2 * (u64)npix));
  const uint32_t* __restrict__ in = staged + (i64)img * npix;
  for (int i = threadIdx.x; i < AUG_HALO * AUG_HALO; i += AUG_NT) {
    const int hy = i / AUG_HALO, hx = i - hy * AUG_HALO, y = ty0 + hy - 1, x = tx0 + hx - 1;
    uint32_t q = 0;                                                     // outside the image: never used (a pixel of the image's border keeps itself)
    if (y >= 0 && y < Ho && x >= 0 && x < Wo) {
      const uint32_t p = in[y * Wo + x];
      int R = blend(mean, p & 255, kc), G = blend(mean, (p >> 8) & 255, kc), B = blend(mean, (p >> 16) & 255, kc);
      const int L = luma(R, G, B);
      R = blend(L, R, ks); G = blend(L, G, ks); B = blend(L, B, ks);
      q = R | (G << 8) | (B << 16);
    }
    tile[hy][hx] = q;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < AUG_PIX; ++k) {
    const int ly = ly0 + k * (AUG_NT / AUG_TILE), y = ty0 + ly, x = tx0 + lx;
    if (y >= Ho || x >= Wo) continue;
    const uint32_t ctr = tile[ly + 1][lx + 1];
    int v[3] = {(int)(ctr & 255), (int)((ctr >> 8) & 255), (int)((ctr >> 16) & 255)};
    if (y > 0 && y < Ho - 1 && x > 0 && x < Wo - 1) {
      int s[3] = {4 * v[0], 4 * v[1], 4 * v[2]};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const uint32_t q = tile[ly + dy][lx + dx];
          s[0] += q & 255; s[1] += (q >> 8) & 255; s[2] += (q >> 16) & 255;
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = blend((2 * s[c] + 13) / 26, v[c], kh);
    }
    const i64 o = ((i64)y * Wo + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (sizeof(T) == 4)
        out[o + c] = (T)((double)v[c] / 255.0);
      else
        out[o + c] = (T)v[c];
    }
  }
}

// ws: the N luma sums, then the staged images, one 32-bit word per pixel
struct AugWs {
  u64* sums;
  uint32_t* staged;
  size_t bytes;
  AugWs(void* ws, int N, int Ho, int Wo) {
    camo_abi::Carver cv(ws);
    sums = cv.take<u64>((size_t)N);
    staged = cv.take<uint32_t>((size_t)N * Ho * Wo);
    bytes = cv.bytes();
  }
};

bool sizes_ok(int N, int C, int Ho, int Wo, int enhance) {
  return N >= 1 && N <= CAMO_RGD_MAX_IMAGES && C >= 1 && C <= CAMO_RSZ_MAX_CHANNELS && Ho >= 1 && Ho <= CAMO_RSZ_MAX_SIDE && Wo >= 1 &&
         Wo <= CAMO_RSZ_MAX_SIDE && (enhance == 0 || (enhance == 1 && C == 3));
}

template <typename T, bool ENH>
int launch_warp(int filter, dim3 grid, hipStream_t st, const uint8_t* src, i64 src_elems, T* dst, const i64* table, int C, int Ho, int Wo, int* status,
                u64* sums) {
  if (filter == CAMO_RSZ_NEAREST)
    hipLaunchKernelGGL((aug_warp_kernel<T, CAMO_RSZ_NEAREST, ENH>), grid, dim3(AUG_NT), 0, st, src, src_elems, dst, table, C, Ho, Wo, status, sums);
  else
    hipLaunchKernelGGL((aug_warp_kernel<T, CAMO_RSZ_BILINEAR, ENH>), grid, dim3(AUG_NT), 0, st, src, src_elems, dst, table, C, Ho, Wo, status, sums);
  return (int)hipGetLastError();
}

}  // namespace

using camo_abi::fail;

extern "C" size_t camo_augment_workspace_bytes(int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t enhance) {
  if (!sizes_ok(N, C, Ho, Wo, enhance) || enhance == 0) return 0;
  return AugWs(nullptr, N, Ho, Wo).bytes;
}

extern "C" int camo_augment(const uint8_t* src, int64_t src_elems, void* dst, int32_t dst_type, const int64_t* table, int32_t N, int32_t C, int32_t Ho,
                            int32_t Wo, int32_t filter, int32_t enhance, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (!src) return fail(CAMO_E_ARG, "src is null");
  if (!dst) return fail(CAMO_E_ARG, "dst is null");
  if (!table) return fail(CAMO_E_ARG, "table is null");
  if (!status) return fail(CAMO_E_ARG, "status is null");
  if (N < 1 || N > CAMO_RGD_MAX_IMAGES) return fail(CAMO_E_ARG, "need 1 <= N <= CAMO_RGD_MAX_IMAGES");
  if (C < 1 || C > CAMO_RSZ_MAX_CHANNELS) return fail(CAMO_E_ARG, "need 1 <= C <= CAMO_RSZ_MAX_CHANNELS");
  if (Ho < 1 || Ho > CAMO_RSZ_MAX_SIDE || Wo < 1 || Wo > CAMO_RSZ_MAX_SIDE) return fail(CAMO_E_ARG, "need Ho, Wo in [1, CAMO_RSZ_MAX_SIDE]");
  if (filter != CAMO_RSZ_NEAREST && filter != CAMO_RSZ_BILINEAR) return fail(CAMO_E_ARG, "filter is neither CAMO_RSZ_NEAREST nor CAMO_RSZ_BILINEAR");
  if (dst_type != CAMO_RSZ_U8 && dst_type != CAMO_RSZ_F32) return fail(CAMO_E_ARG, "dst_type is neither CAMO_RSZ_U8 nor CAMO_RSZ_F32");
  if (enhance != 0 && enhance != 1) return fail(CAMO_E_ARG, "enhance is neither 0 nor 1");
  if (enhance == 1 && C != 3) return fail(CAMO_E_ARG, "enhance = 1 needs C = 3");
  if (src_elems < 1) return fail(CAMO_E_ARG, "need src_elems >= 1");
  if (dst_type == CAMO_RSZ_F32 && (reinterpret_cast<uintptr_t>(dst) & 3)) return fail(CAMO_E_ARG, "an fp32 dst must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(table) & 7) return fail(CAMO_E_ARG, "table must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(status) & 3) return fail(CAMO_E_ARG, "status must be 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const i64* tb = reinterpret_cast<const i64*>(table);
  const dim3 grid((unsigned)((Ho * Wo + AUG_NT * AUG_PIX - 1) / (AUG_NT * AUG_PIX)), (unsigned)N);
  if (enhance == 0) {
    if (dst_type == CAMO_RSZ_F32)
      CK((launch_warp<float, false>(filter, grid, st, src, src_elems, static_cast<float*>(dst), tb, C, Ho, Wo, status, nullptr)), "augment warp");
    else
      CK((launch_warp<uint8_t, false>(filter, grid, st, src, src_elems, static_cast<uint8_t*>(dst), tb, C, Ho, Wo, status, nullptr)), "augment warp");
    return 0;
  }
  if (!ws) return fail(CAMO_E_ARG, "ws is null");
  const AugWs w(ws, N, Ho, Wo);
  if (int e = camo_abi::ws_check(ws, ws_bytes, w.bytes, "camo_augment_workspace_bytes")) return e;
  hipLaunchKernelGGL(aug_clear_kernel, dim3((unsigned)((N + AUG_NT - 1) / AUG_NT)), dim3(AUG_NT), 0, st, w.sums, (int)N);
  CK((int)hipGetLastError(), "augment clear");
  CK((launch_warp<uint32_t, true>(filter, grid, st, src, src_elems, w.staged, tb, C, Ho, Wo, status, w.sums)), "augment warp");
  const int tiles_x = (Wo + AUG_TILE - 1) / AUG_TILE, tiles_y = (Ho + AUG_TILE - 1) / AUG_TILE;
  const dim3 egrid((unsigned)(tiles_x * tiles_y), (unsigned)N);
  if (dst_type == CAMO_RSZ_F32)
    hipLaunchKernelGGL((aug_enhance_kernel<float>), egrid, dim3(AUG_NT), 0, st, w.staged, w.sums, static_cast<float*>(dst), tb, (int)Ho, (int)Wo, tiles_x, status);
  else
    hipLaunchKernelGGL((aug_enhance_kernel<uint8_t>), egrid, dim3(AUG_NT), 0, st, w.staged, w.sums, static_cast<uint8_t*>(dst), tb, (int)Ho, (int)Wo, tiles_x, status);
  CK((int)hipGetLastError(), "augment enhance");
  return 0;
}
