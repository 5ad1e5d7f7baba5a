// Edge-aware mask refinement (include/camo_guided.h): the guided filter at the working size and the application of its
// coefficients to native-size 8-bit guides.  The header's text is the definition.  Everything between the fp32 inputs and the fp32
// outputs is FP64 vector arithmetic on purpose: the one-pass covariance mean(I I) - mu mu cancels, and in float the result is off by a
// thousand times the rounding of the outputs.  One thread computes one output element in a fixed order: no atomics, no reduction
// across threads, the same bytes every call.
//
//   rows_in    per pixel the clipped ROW sums of the 4 (grey) / 13 (colour) planes I_c, p, I_c p, I_i I_j, the products formed on the
//              fly from the fp32 inputs (exact in double) -> ws.sums, plane-major so that the next kernel's lanes read along a row
//   cols_solve per pixel the clipped COLUMN sums of those, the means, the C x C solve -> a_c, b (double) -> ws.ab
//   rows_ab    the row sums of a_c, b -> ws.sums
//   cols_out   their column sums, the means abar_c, bbar -> coef (fp32), q = abar . I + bbar (from the doubles) -> q (fp32)
//   apply      camo_resize's bilinear taps on the C + 1 coefficient planes, kept in double, times the native u8 pixel -> fp32
#include <hip/hip_runtime.h>

#include "abi_util.h"
#include "guided.h"
#include "resize_taps.h"
#include "../../include/camo_guided.h"

namespace {

typedef long long i64;
constexpr int NT = GF_NT;

// A pixel of the batch: image n, row y, column x, and the clipped window's ends along one axis.
struct Pix { int n, y, x; i64 hw, at; };      // at = y W + x

__device__ __forceinline__ bool locate(i64 total, int H, int W, Pix& p) {
  const i64 idx = (i64)blockIdx.x * NT + threadIdx.x;
  if (idx >= total) return false;
  p.hw = (i64)H * W;
  p.n = (int)(idx / p.hw);
  p.at = idx - p.n * p.hw;
  p.y = (int)(p.at / W);
  p.x = (int)(p.at - (i64)p.y * W);
  return true;
}

template <int C>
__global__ __launch_bounds__(NT) void gf_rows_in(const float* __restrict__ guide, const float* __restrict__ p, i64 p_stride, i64 total, int H, int W,
                                                 int r, double* __restrict__ sums) {
  constexpr int K = gf_sum_planes(C);
  Pix px;
  if (!locate(total, H, W, px)) return;
  const int x0 = max(px.x - r, 0), x1 = min(px.x + r, W - 1);
  const float* __restrict__ grow = guide + ((i64)px.n * px.hw + (i64)px.y * W) * C;
  const float* __restrict__ prow = p + (i64)px.n * p_stride + (i64)px.y * W;
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.0;
  for (int xx = x0; xx <= x1; ++xx) {
    const double pv = (double)prow[xx];
    double g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = (double)grow[(i64)xx * C + c];
#pragma unroll
    for (int c = 0; c < C; ++c) { s[c] += g[c]; s[C + 1 + c] += g[c] * pv; }
    s[C] += pv;
    int k = 2 * C + 1;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
      for (int j = i; j < C; ++j) s[k++] += g[i] * g[j];
  }
  double* __restrict__ o = sums + (i64)px.n * K * px.hw + px.at;
#pragma unroll
  for (int k = 0; k < K; ++k) o[(i64)k * px.hw] = s[k];
}

// the clipped column sums of `planes` row-sum planes of image n at column x -> s[]
template <int PLANES>
__device__ __forceinline__ void column_sums(const double* __restrict__ img, i64 hw, int W, int x, int y0, int y1, double (&s)[PLANES]) {
#pragma unroll
  for (int k = 0; k < PLANES; ++k) s[k] = 0.0;
  for (int yy = y0; yy <= y1; ++yy) {
    const double* __restrict__ at = img + (i64)yy * W + x;
#pragma unroll
    for (int k = 0; k < PLANES; ++k) s[k] += at[(i64)k * hw];
  }
}

template <int C>
__global__ __launch_bounds__(NT) void gf_cols_solve(const double* __restrict__ sums, i64 total, int H, int W, int r, double eps, double* __restrict__ ab) {
  constexpr int K = gf_sum_planes(C);
  Pix px;
  if (!locate(total, H, W, px)) return;
  const int y0 = max(px.y - r, 0), y1 = min(px.y + r, H - 1), x0 = max(px.x - r, 0), x1 = min(px.x + r, W - 1);
  double s[K];
  column_sums<K>(sums + (i64)px.n * K * px.hw, px.hw, W, px.x, y0, y1, s);
  const double cnt = (double)((y1 - y0 + 1) * (x1 - x0 + 1));
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = s[k] / cnt;
  double* __restrict__ o = ab + (i64)px.n * (C + 1) * px.hw + px.at;
  const double pbar = s[C];
  if constexpr (C == 1) {
    const double mu = s[0];
    const double a = (s[2] - mu * pbar) / (s[3] - mu * mu + eps);
    o[0] = a;
    o[px.hw] = pbar - a * mu;
  } else {
    const double m0 = s[0], m1 = s[1], m2 = s[2];
    const double c0 = s[4] - m0 * pbar, c1 = s[5] - m1 * pbar, c2 = s[6] - m2 * pbar;
    const double M00 = s[7] - m0 * m0 + eps, M01 = s[8] - m0 * m1, M02 = s[9] - m0 * m2;
    const double M11 = s[10] - m1 * m1 + eps, M12 = s[11] - m1 * m2, M22 = s[12] - m2 * m2 + eps;
    const double A00 = M11 * M22 - M12 * M12, A01 = M02 * M12 - M01 * M22, A02 = M01 * M12 - M02 * M11;
    const double A11 = M00 * M22 - M02 * M02, A12 = M01 * M02 - M00 * M12, A22 = M00 * M11 - M01 * M01;
    const double det = M00 * A00 + M01 * A01 + M02 * A02;
    const double a0 = (A00 * c0 + A01 * c1 + A02 * c2) / det;
    const double a1 = (A01 * c0 + A11 * c1 + A12 * c2) / det;
    const double a2 = (A02 * c0 + A12 * c1 + A22 * c2) / det;
    o[0] = a0; o[px.hw] = a1; o[2 * px.hw] = a2;
    o[3 * px.hw] = pbar - (a0 * m0 + a1 * m1 + a2 * m2);
  }
}

template <int C>
__global__ __launch_bounds__(NT) void gf_rows_ab(const double* __restrict__ ab, i64 total, int H, int W, int r, double* __restrict__ sums) {
  Pix px;
  if (!locate(total, H, W, px)) return;
  const int x0 = max(px.x - r, 0), x1 = min(px.x + r, W - 1);
  const i64 base = (i64)px.n * (C + 1) * px.hw + (i64)px.y * W;
  double s[C + 1];
#pragma unroll
  for (int k = 0; k <= C; ++k) s[k] = 0.0;
  for (int xx = x0; xx <= x1; ++xx) {
#pragma unroll
    for (int k = 0; k <= C; ++k) s[k] += ab[base + (i64)k * px.hw + xx];
  }
#pragma unroll
  for (int k = 0; k <= C; ++k) sums[base + (i64)k * px.hw + px.x] = s[k];
}

template <int C>
__global__ __launch_bounds__(NT) void gf_cols_out(const double* __restrict__ sums, const float* __restrict__ guide, i64 total, int H, int W, int r,
                                                  int clamp, float* __restrict__ q, float* __restrict__ coef) {
  Pix px;
  if (!locate(total, H, W, px)) return;
  const int y0 = max(px.y - r, 0), y1 = min(px.y + r, H - 1), x0 = max(px.x - r, 0), x1 = min(px.x + r, W - 1);
  double s[C + 1];
  column_sums<C + 1>(sums + (i64)px.n * (C + 1) * px.hw, px.hw, W, px.x, y0, y1, s);
  const double cnt = (double)((y1 - y0 + 1) * (x1 - x0 + 1));
#pragma unroll
  for (int k = 0; k <= C; ++k) s[k] = s[k] / cnt;
  const float* __restrict__ g = guide + ((i64)px.n * px.hw + px.at) * C;
  double v = s[0] * (double)g[0];
#pragma unroll
  for (int c = 1; c < C; ++c) v += s[c] * (double)g[c];
  v += s[C];
  if (clamp) v = fmin(fmax(v, 0.0), 1.0);
  q[(i64)px.n * px.hw + px.at] = (float)v;
  if (coef) {
    float* __restrict__ o = coef + (i64)px.n * (C + 1) * px.hw + px.at;
#pragma unroll
    for (int k = 0; k <= C; ++k) o[(i64)k * px.hw] = (float)s[k];
  }
}

// camo_guided_apply.  The row checks come first, as in resize.hip: a wrong table can neither read nor write outside the buffers.
template <int C>
__global__ __launch_bounds__(NT) void gf_apply(const float* __restrict__ coef, int h, int w, const uint8_t* __restrict__ guide, i64 guide_elems,
                                               float* __restrict__ out, i64 out_elems, const i64* __restrict__ table, i64 max_dst_pixels, int clamp,
                                               int* __restrict__ status) {
  const int img = blockIdx.y;
  const i64* __restrict__ row = table + (i64)img * CAMO_GF_FIELDS;
  const i64 g_off = row[0], H = row[1], W = row[2], o_off = row[3];
  const bool dst_form = o_off >= 0 && rsz::side_ok(H) && rsz::side_ok(W) && H * W <= max_dst_pixels;      // (H W <= 2^26: no overflow below)
  const bool ok = dst_form && g_off >= 0 && H * W * C <= guide_elems && g_off <= guide_elems - H * W * C && H * W <= out_elems &&
                  o_off <= out_elems - H * W;
  if (threadIdx.x == 0) status[img] = ok ? 0 : 1;
  if (!dst_form) return;
  const int DH = (int)H, DW = (int)W, npix = DH * DW;
  const int first = blockIdx.x * (NT * GF_APPLY_PIX) + threadIdx.x;
  if (first - (int)threadIdx.x >= npix) return;

  if (!ok) {                                                  // zeros over the stated destination where it lies inside out; nothing is read
    for (int k = 0; k < GF_APPLY_PIX; ++k) {
      const int pix = first + k * NT;
      if (pix >= npix) return;
      i64 e;
      if (__builtin_add_overflow(o_off, (i64)pix, &e)) continue;
      if (e < out_elems) out[e] = 0.f;
    }
    return;
  }

  const i64 hw = (i64)h * w;
  const float* __restrict__ cf = coef + (i64)img * (C + 1) * hw;
  const uint8_t* __restrict__ gb = guide + g_off;
  const i64 groom = guide_elems - g_off;
#pragma unroll
  for (int k = 0; k < GF_APPLY_PIX; ++k) {                    // independent pixels with no branch between them: their loads are in flight together
    const int at = first + k * NT, pix = min(at, npix - 1);   // (past the image: the last pixel once more, and no store)
    const int y = pix / DW, x = pix - y * DW;
    const rsz::Axis ay = rsz::make_axis<CAMO_RSZ_BILINEAR>(0, h, DH, y, false);
    const rsz::Axis ax = rsz::make_axis<CAMO_RSZ_BILINEAR>(0, w, DW, x, false);
    int sy0, wy0, sx0, wx0, sy1, wy1, sx1, wx1;
    rsz::tap(ay, 0, sy0, wy0); rsz::tap(ay, 1, sy1, wy1);
    rsz::tap(ax, 0, sx0, wx0); rsz::tap(ax, 1, sx1, wx1);
    const double w00 = (double)(wy0 * wx0), w01 = (double)(wy0 * wx1), w10 = (double)(wy1 * wx0), w11 = (double)(wy1 * wx1);
    const double den = (double)((i64)ay.T * ax.T);
    const float* __restrict__ r0 = cf + (i64)sy0 * w;
    const float* __restrict__ r1 = cf + (i64)sy1 * w;
    double s[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) {
      const i64 co = (i64)c * hw;
      double acc = w00 * (double)r0[co + sx0];                // exact products (header): an FMA below rounds as multiply-then-add does
      acc += w01 * (double)r0[co + sx1];
      acc += w10 * (double)r1[co + sx0];
      acc += w11 * (double)r1[co + sx1];
      s[c] = acc / den;
    }
    int v[CAMO_RSZ_MAX_CHANNELS];
    const i64 go = (i64)pix * C;
    rsz::load_bytes(gb + go, groom - go, 1, C, v);
    double qv = s[0] * ((double)v[0] / 255.0);
#pragma unroll
    for (int c = 1; c < C; ++c) qv += s[c] * ((double)v[c] / 255.0);
    qv += s[C];
    if (clamp) qv = fmin(fmax(qv, 0.0), 1.0);
    if (at < npix) out[o_off + pix] = (float)qv;
  }
}

}  // namespace

GfWs gf_carve(int N, int H, int W, int C, void* base) {
  GfWs ws{};
  camo_abi::Carver c(base);
  const size_t npix = (size_t)N * H * W;
  ws.sums = c.take<double>(npix * gf_sum_planes(C));
  ws.ab = c.take<double>(npix * (C + 1));
  ws.bytes = c.bytes();
  return ws;
}

template <int C>
static int filter_launches(const float* guide, const float* p, i64 p_stride, int N, int H, int W, int r, double eps, bool clamp, float* q,
                           float* coef, const GfWs& ws, hipStream_t st) {
  const i64 total = (i64)N * H * W;
  const dim3 grid((unsigned)((total + NT - 1) / NT)), block(NT);
  hipLaunchKernelGGL(gf_rows_in<C>, grid, block, 0, st, guide, p, p_stride, total, H, W, r, ws.sums);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(gf_cols_solve<C>, grid, block, 0, st, ws.sums, total, H, W, r, eps, ws.ab);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(gf_rows_ab<C>, grid, block, 0, st, ws.ab, total, H, W, r, ws.sums);
  if (int e = (int)hipGetLastError()) return e;
  hipLaunchKernelGGL(gf_cols_out<C>, grid, block, 0, st, ws.sums, guide, total, H, W, r, clamp ? 1 : 0, q, coef);
  return (int)hipGetLastError();
}

int launch_guided_filter(const float* guide, const float* p, long long p_stride, int N, int H, int W, int C, int radius, double eps, bool clamp,
                         float* q, float* coef, const GfWs& ws, hipStream_t stream) {
  return C == 1 ? filter_launches<1>(guide, p, p_stride, N, H, W, radius, eps, clamp, q, coef, ws, stream)
                : filter_launches<3>(guide, p, p_stride, N, H, W, radius, eps, clamp, q, coef, ws, stream);
}

int launch_guided_apply(const float* coef, int N, int C, int h, int w, const unsigned char* guide, long long guide_elems, float* out,
                        long long out_elems, const long long* table, long long max_dst_pixels, bool clamp, int* status, hipStream_t stream) {
  const dim3 grid((unsigned)((max_dst_pixels + NT * GF_APPLY_PIX - 1) / (NT * GF_APPLY_PIX)), (unsigned)N), block(NT);
  if (C == 1)
    hipLaunchKernelGGL(gf_apply<1>, grid, block, 0, stream, coef, h, w, guide, guide_elems, out, out_elems, table, max_dst_pixels, clamp ? 1 : 0, status);
  else
    hipLaunchKernelGGL(gf_apply<3>, grid, block, 0, stream, coef, h, w, guide, guide_elems, out, out_elems, table, max_dst_pixels, clamp ? 1 : 0, status);
  return (int)hipGetLastError();
}
