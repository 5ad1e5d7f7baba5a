// Head-averaged attention maps behind the fused row-tile forward (attn_maps.h).
//
// The fused forward keeps its probabilities on chip, so a call that wants the maps recomputes them from what the front half left
// in the workspace.  Per packed RG row r of sample b, head h, KG row k < Nk:
//   rg2kg[r, k] = 1/8 sum_h softmax_k(q_h[r] . k_h[k])                  q: Q16 (pre-scaled), k: the K half of the sample's KV16 rows
//   kg2rg[r, k] = 1/8 sum_h exp(q2_h[k] . k2_h[r] - M[h, k]) / L[h, k]  q2: Q2_16 (pre-scaled), k2: the K half of KV2_16 row r,
//                                                                        {M, L}: the back half's softmax statistics (lse2)
// i.e. the probabilities the forward's PV products used, before their rounding to bf16.  No row needs another row of its sample, so
// the launch is one block per 32-row tile of the batch descriptor's table (a tile never crosses a sample): 6.7 k MACs against 1 KB
// read and 104 B written per row -- a bandwidth kernel, on the VALU (v_dot2_f32_bf16 straight from the packed operands).
//
// Thread (r = tid & 31, h = tid >> 5) owns one (row, head): its 32 q and 32 k2 values stay in 32 VGPRs as packed bf16, the sample's
// keys and KG queries (Nk x 512 B each) sit in LDS where the 32 lanes of a head read the same address (broadcast).  A wave's loads
// cover 128 contiguous bytes (two heads) of 32 consecutive rows: whole cache lines.  The 8 heads of a row meet in LDS, and the
// tile's [rows][Nk] outputs leave as one contiguous run of dword stores.  Rows past the tile's end and keys past Nk are never read.
#include "attn_maps.h"
#include "gemm.h"
#include "mfma_inl.h"   // u32x4

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// c + a.lo * b.lo + a.hi * b.hi on two packed bf16 pairs, fp32 accumulate
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
#if __has_builtin(__builtin_amdgcn_fdot2_f32_bf16)
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), c, false);
#else
  c = fmaf(__uint_as_float(a << 16), __uint_as_float(b << 16), c);
  return fmaf(__uint_as_float(a & 0xFFFF0000u), __uint_as_float(b & 0xFFFF0000u), c);
#endif
}
__device__ __forceinline__ float dot8(const u32x4& a, const u32x4& b, float c) {
  c = dot2(a[0], b[0], c); c = dot2(a[1], b[1], c); c = dot2(a[2], b[2], c);
  return dot2(a[3], b[3], c);
}

constexpr int PS = 8 * 32 + 1;       // floats per key of a probability tile [16 keys][8 heads][32 rows] (+1: the readers walk keys first)

__global__ __launch_bounds__(256) void attn_maps_kernel(const AttnMapsArgs a) {
  __shared__ __attribute__((aligned(16))) us16 Ks[16 * 256];      // the sample's keys  [k][256]  (rows >= Nk: zero)
  __shared__ __attribute__((aligned(16))) us16 Q2s[16 * 256];     // the sample's KG queries
  __shared__ float Ms[128], iLs[128];                             // [head][query]: softmax maximum, 1 / sum
  __shared__ float P1[16 * PS], P2[16 * PS];
  const int4 td = a.tile_desc[blockIdx.x];
  if (td.x < 0) return;                                           // (block-uniform: surplus tiles of the table)
  const int b = td.x, row0 = td.y, nrows = td.z, Nk = a.Nk;
  const int tid = threadIdx.x, r = tid & 31, h = tid >> 5;
  const bool live = r < nrows;
  // this thread's operands: 64 bytes of its row's queries and of its row's keys (head h)
  u32x4 q[4], k2[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) { q[c] = u32x4{0u, 0u, 0u, 0u}; k2[c] = u32x4{0u, 0u, 0u, 0u}; }
  if (live) {
    const us16* qp = a.Q16 + (size_t)(row0 + r) * 256 + 32 * h;
    const us16* kp = a.KV2_16 + (size_t)(row0 + r) * 512 + 32 * h;
#pragma unroll
    for (int c = 0; c < 4; ++c) { q[c] = *reinterpret_cast<const u32x4*>(qp + 8 * c); k2[c] = *reinterpret_cast<const u32x4*>(kp + 8 * c); }
  }
  // the sample's side: 16 rows x 32 chunks of 16 bytes per tensor, two chunks per thread
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = tid + 256 * i, k = c >> 5, o = 8 * (c & 31);
    u32x4 kv = u32x4{0u, 0u, 0u, 0u}, qv = u32x4{0u, 0u, 0u, 0u};
    if (k < Nk) {
      kv = *reinterpret_cast<const u32x4*>(a.KV16 + ((size_t)b * Nk + k) * 512 + o);
      qv = *reinterpret_cast<const u32x4*>(a.Q2_16 + ((size_t)b * Nk + k) * 256 + o);
    }
    *reinterpret_cast<u32x4*>(Ks + k * 256 + o) = kv;
    *reinterpret_cast<u32x4*>(Q2s + k * 256 + o) = qv;
  }
  if (tid < 128) {
    const int j = tid & 15;                                        // tid = head * 16 + query
    const float* s = a.lse2 + ((size_t)b * 128 + tid) * 2;
    Ms[tid] = j < Nk ? s[0] : 0.f;
    iLs[tid] = j < Nk ? 1.0f / s[1] : 0.f;
  }
  __syncthreads();
  float s1[16], s2[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    s1[k] = 0.f; s2[k] = 0.f;
    if (k < Nk) {                                                  // (block-uniform)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s1[k] = dot8(q[c], *reinterpret_cast<const u32x4*>(Ks + k * 256 + 32 * h + 8 * c), s1[k]);
        s2[k] = dot8(k2[c], *reinterpret_cast<const u32x4*>(Q2s + k * 256 + 32 * h + 8 * c), s2[k]);
      }
    }
  }
  float m = -INFINITY, l = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) m = k < Nk ? fmaxf(m, s1[k]) : m;
#pragma unroll
  for (int k = 0; k < 16; ++k) { s1[k] = k < Nk ? __expf(s1[k] - m) : 0.f; l += s1[k]; }
  const float il = 1.0f / l;
  if (live) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < Nk) {
        P1[k * PS + 32 * h + r] = s1[k] * il;
        P2[k * PS + 32 * h + r] = __expf(s2[k] - Ms[16 * h + k]) * iLs[16 * h + k];
      }
  }
  __syncthreads();
  // head average: output o = (row o / Nk, key o % Nk) of the tile's contiguous [nrows][Nk] run
  const size_t out0 = (size_t)row0 * Nk;
  for (int o = tid; o < nrows * Nk; o += 256) {
    const int rr = o / Nk, k = o - rr * Nk;
    const float* p1 = P1 + k * PS + rr; const float* p2 = P2 + k * PS + rr;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int hd = 0; hd < 8; ++hd) { a1 += p1[32 * hd]; a2 += p2[32 * hd]; }
    if (a.rg2kg) a.rg2kg[out0 + o] = a1 * 0.125f;
    if (a.kg2rg) a.kg2rg[out0 + o] = a2 * 0.125f;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int launch_attn_maps(const AttnMapsArgs& a, hipStream_t stream) {
  if (a.Nk < 1 || a.Nk > 16 || a.tiles < 1 || !a.Q16 || !a.KV16 || !a.Q2_16 || !a.KV2_16 || !a.lse2 || !a.tile_desc || (!a.rg2kg && !a.kg2rg))
    return (int)hipErrorInvalidValue;
  if (!al16(a.Q16) || !al16(a.KV16) || !al16(a.Q2_16) || !al16(a.KV2_16) || !al16(a.tile_desc)) return (int)hipErrorInvalidValue;
  // executed FLOPs: two score products of Nk x 256 MACs per row
  const int prof = gemm_prof_open(stream, 2.0 * (double)a.rows_rg * a.Nk * 256.0 * 2.0, PROF_ATTN);
  hipLaunchKernelGGL(attn_maps_kernel, dim3(a.tiles), dim3(256), 0, stream, a);
  gemm_prof_close(prof, stream);
  return (int)hipGetLastError();
}
