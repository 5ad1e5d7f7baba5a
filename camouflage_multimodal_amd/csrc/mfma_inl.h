// The fused kernels' shared device vocabulary (gfx950): MFMA fragment types and conversions, the accumulator-layout rule, the
// write-through tile store, the RG row softmax and the LDS tile pitches.  Every kernel family (fused_rows.hip, fused_wide.hip,
// wide2_inl.h, tail_wide.hip, gemm16.hip) takes them from here; the layouts are stated executably in tests/test_fragment_maps.py.
// Everything sits in an anonymous namespace: include once per translation unit.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));      // one 32x32 accumulator tile
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));       // one operand fragment of v_mfma_f32_32x32x16_bf16
typedef short s16x4 __attribute__((ext_vector_type(4)));        // half a fragment: what one transposing LDS read returns
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bf16x8 as_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ s16x4 lds_tr16(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
__device__ __forceinline__ bf16x8 join(s16x4 lo, s16x4 hi) { return bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}; }
__device__ __forceinline__ f32x16 splat16(float v) {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = v;
  return z;
}
__device__ __forceinline__ f32x16 zero16() { return splat16(0.f); }
// the two bf16 of a packed dword (pack2, common.h) as floats
__device__ __forceinline__ float bf_lo(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float bf_hi(uint32_t v) { return __uint_as_float(v & 0xFFFF0000u); }
// accumulator register r of lane half h holds row (r & 3) + 8 (r >> 2) + 4 h of the 32x32 tile
__device__ __forceinline__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// 16-byte write-through store (sc0 sc1): the bytes go to memory as they are issued instead of staying dirty in this XCD's L2
// until the end-of-kernel write-back, which then has that much less to do before the next launch may start
// (tile outputs of one training step: ~60 MB; measured -2.5 us per step at B = 16).
// s_nop: the data registers may be rewritten right behind an asm store (the compiler's hazard pass covers its own instructions only).
__device__ __forceinline__ void store16_wt(void* p, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// Softmax over the <= 16 keys of one RG row: S holds the (pre-scaled) scores of keys acc_row(i, h), i < 8, in this lane
// and the other 8 keys in lane ^ 32.  p = probabilities (0 for keys >= Nk).  The forward kernels, the backward kernels (which
// recompute the probabilities the forward used) and the attention maps' consumers all run THIS code: one definition keeps them
// bit-identical.
__device__ __forceinline__ void rg_softmax(const f32x16& S, int h, int Nk, float (&p)[8]) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) { p[i] = acc_row(i, h) < Nk ? S[i] : -INFINITY; m = fmaxf(m, p[i]); }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { p[i] = __expf(p[i] - m); sum += p[i]; }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
#pragma unroll
  for (int i = 0; i < 8; ++i) p[i] *= inv;
}

// Row pitches (bytes) of the bf16 tiles in LDS.  PX, PR, PQ: the dense row + 16 bytes, so consecutive rows start 4 banks apart and a
// ds_read_b128 lane group's 16 rows land on 16 distinct bank quads.
constexpr int PX = 272;      // [rows][128] tile (the input)
constexpr int PR = 528;      // [rows][256] tile
constexpr int PQ = 1552;     // [rows][768] tile [q | k' | v']
constexpr int PV = 576;      // the 16 value rows of a sample [16][256]: dense row + 64 bytes (transposing reads: rows 16 banks apart)

}  // namespace
