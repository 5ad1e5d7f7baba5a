// Canny edge maps of a batch of images: skimage.feature.canny(gray, sigma) as the reference calls it
// (models/region_graph/extract_rg_embeddings.py:151-152), restated in include/camo_canny.h.  0.8 MB in and 64 KB out per
// 256 x 256 image: the work is launches and latency, so every grid covers the whole batch and there are five launches.
//
//   gradient     one block per 32 x 32 tile: luma with a halo of radius + 1 in LDS (zero outside the image), Gaussian
//                rows then columns in LDS, division by the blur of an all-ones image (a row factor times a column
//                factor), 3 x 3 Sobel on the smoothed tile with the border pixel repeated -> gi, gj, magnitude
//   label tiles  one block per tile: class of each pixel (interpolated non-maximum suppression + the two thresholds,
//                fp32 without contraction), then the 8-connected components of the tile's weak pixels in LDS (cc_inl.h):
//                every weak pixel points at the smallest index of its component inside the tile
//   join tiles   weak pixels on a tile border: cc_inl.h's unions with their neighbours in other tiles, on the global labels
//   flag         every weak pixel finds its root and points at it; strong pixels set flag[root]
//   emit         edges = weak and flag[root]
//
// A component's root is its smallest index whatever the order the unions ran in (cc_inl.h), so the output depends on the
// partition alone.
#include <hip/hip_runtime.h>
#include "abi_util.h"
#include "canny.h"
#include "cc_inl.h"

namespace {

constexpr int T = CANNY_TILE, T2 = CANNY_TILE + 2, NT = 256;

__global__ __launch_bounds__(NT) void canny_gradient_kernel(const float* __restrict__ images, int H, int W, CannyTaps taps,
                                                            float* __restrict__ grad) {
  extern __shared__ float lds[];
  const int R = taps.radius, S = T2 + 2 * R;
  float* luma = lds;                  // [S][S]   image rows y0 - 1 - R .., columns x0 - 1 - R ..
  float* rowb = luma + S * S;         // [S][T2]  blurred along x, columns x0 - 1 ..
  float* sm = rowb + S * T2;          // [T2][T2] smoothed image, rows y0 - 1 .., columns x0 - 1 ..
  float* rf = sm + T2 * T2;           // [T2] blur of ones along y at rows y0 - 1 ..
  float* cf = rf + T2;                // [T2] ... along x
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const float* img = images + (size_t)n * H * W * 3;
  for (int i = tid; i < S * S; i += NT) {
    const int ly = i / S, lx = i - ly * S, y = y0 - 1 - R + ly, x = x0 - 1 - R + lx;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const float* p = img + ((size_t)y * W + x) * 3;
      v = 0.2989f * p[0] + 0.5870f * p[1] + 0.1140f * p[2];
    }
    luma[i] = v;
  }
  if (tid < 2 * T2) {
    const bool row = tid < T2;
    const int t = row ? tid : tid - T2, c = (row ? y0 : x0) - 1 + t, len = row ? H : W;
    float s = 0.f;
    for (int k = -R; k <= R; ++k)
      if (c + k >= 0 && c + k < len) s += taps.w[k + R];
    (row ? rf : cf)[t] = s;
  }
  __syncthreads();
  for (int i = tid; i < S * T2; i += NT) {
    const int ly = i / T2, tx = i - ly * T2;
    const float* src = luma + ly * S + tx;
    float s = 0.f;
    for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * src[k];
    rowb[i] = s;
  }
  __syncthreads();
  for (int i = tid; i < T2 * T2; i += NT) {
    const int ty = i / T2, tx = i - ty * T2;
    const float* src = rowb + ty * T2 + tx;
    float s = 0.f;
    for (int k = 0; k <= 2 * R; ++k) s += taps.w[k] * src[k * T2];
    sm[i] = s / (rf[ty] * cf[tx] + 2.220446049250313e-16f);
  }
  __syncthreads();
  const size_t HW = (size_t)H * W;
  float* g = grad + (size_t)n * 3 * HW;
  for (int i = tid; i < T * T; i += NT) {
    const int oy = i / T, ox = i - oy * T, y = y0 + oy, x = x0 + ox;
    if (y >= H || x >= W) continue;
    // rows / columns of sm for y - 1, y, y + 1 with the border pixel repeated (scipy.ndimage mode="reflect" at width 3)
    const int ru = max(y - 1, 0) - y0 + 1, rc = oy + 1, rd = min(y + 1, H - 1) - y0 + 1;
    const int cl = max(x - 1, 0) - x0 + 1, cc = ox + 1, cr = min(x + 1, W - 1) - x0 + 1;
    const float ul = sm[ru * T2 + cl], uc = sm[ru * T2 + cc], ur = sm[ru * T2 + cr];
    const float ml = sm[rc * T2 + cl], mr = sm[rc * T2 + cr];
    const float dl = sm[rd * T2 + cl], dc = sm[rd * T2 + cc], dr = sm[rd * T2 + cr];
    const float gi = (dl + 2.f * dc + dr) - (ul + 2.f * uc + ur);
    const float gj = (ur + 2.f * mr + dr) - (ul + 2.f * ml + dl);
    const size_t p = (size_t)y * W + x;
    g[p] = gi; g[HW + p] = gj; g[2 * HW + p] = sqrtf(gi * gi + gj * gj);
  }
}

// class of pixel (y, x) from one image's [3][H][W] gradients: include/camo_canny.h step 4, in its operation order
__device__ __forceinline__ int canny_classify(const float* __restrict__ g, int y, int x, int H, int W, float low, float high) {
  if (y < 1 || x < 1 || y >= H - 1 || x >= W - 1) return 0;
  const long long HW = (long long)H * W, p = (long long)y * W + x;
  const float* M = g + 2 * HW;
  const float gi = g[p], gj = g[HW + p], m = M[p];
  if (!(m >= low)) return 0;
  const int s = ((gi > 0.f && gj > 0.f) || (gi < 0.f && gj < 0.f) || gi == 0.f || gj == 0.f) ? 1 : -1;
  const float ai = fabsf(gi), aj = fabsf(gj);
  float a, b, f1, f2, b1, b2;
  if (ai >= aj) { a = aj; b = ai; f1 = M[p + W]; f2 = M[p + W + s]; b1 = M[p - W]; b2 = M[p - W - s]; }
  else          { a = ai; b = aj; f1 = M[p + s]; f2 = M[p + W + s]; b1 = M[p - s]; b2 = M[p - W - s]; }
  bool keep;
  {
#pragma clang fp contract(off)
    const float d = b - a, rhs = m * b;
    const float tf = f2 * a, uf = f1 * d, lf = tf + uf;
    const float tb = b2 * a, ub = b1 * d, lb = tb + ub;
    keep = lf <= rhs && lb <= rhs;
  }
  return keep ? (m >= high ? 2 : 1) : 0;
}

template <bool CLASSIFY>
__global__ __launch_bounds__(NT) void canny_label_tiles_kernel(const float* __restrict__ grad, const unsigned char* __restrict__ cls_in,
                                                               unsigned char* __restrict__ cls_out, float low, float high, int H, int W,
                                                               int* __restrict__ label, unsigned char* __restrict__ flag) {
  __shared__ int lab[T * T];
  const int tid = threadIdx.x, n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t HW = (size_t)H * W, base = (size_t)n * HW;
  for (int l = tid; l < T * T; l += NT) {
    const int y = y0 + l / T, x = x0 + l % T;
    int c = 0;
    if (y < H && x < W) {
      const size_t p = base + (size_t)y * W + x;
      if (CLASSIFY) { c = canny_classify(grad + 3 * base, y, x, H, W, low, high); cls_out[p] = (unsigned char)c; }
      else c = cls_in[p];
      flag[p] = 0;
    }
    lab[l] = cc_run_parent<T, NT>(l, c != 0, cc_all{});
  }
  __syncthreads();
  for (int l = tid; l < T * T; l += NT) cc_tile_unions<8, T>(lab, l, cc_all{});
  __syncthreads();
  for (int l = tid; l < T * T; l += NT) {
    const int y = y0 + l / T, x = x0 + l % T;
    if (y >= H || x >= W) continue;
    label[base + (size_t)y * W + x] = lab[l] >= 0 ? cc_tile_root<T>(lab, l, base, y0, x0, W) : -1;
  }
}

__global__ __launch_bounds__(NT) void canny_join_tiles_kernel(int* label, int N, int H, int W) {
  const long long total = (long long)N * H * W, p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  // (a weak pixel's label was written by the launch before and stays >= 0)
  cc_join_borders<8, T>(label, p, H, W, [label](long long q) { return label[q] >= 0; }, cc_all{});
}

__global__ __launch_bounds__(NT) void canny_flag_kernel(int* label, const unsigned char* __restrict__ cls, unsigned char* flag, long long total) {
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  if (label[p] < 0) return;
  const int r = cc_flatten(label, p);
  if (cls[p] >= 2) flag[r] = 1;                                 // (every writer stores the same byte)
}

__global__ __launch_bounds__(NT) void canny_emit_kernel(const int* __restrict__ label, const unsigned char* __restrict__ flag,
                                                        unsigned char* __restrict__ edges, long long total) {
  const long long p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  int r = label[p];
  if (r >= 0)
    for (int q; (q = label[r]) != r;) r = q;
  edges[p] = (r >= 0 && flag[r]) ? 1 : 0;
}

}  // namespace

CannyWs canny_carve(size_t npix, void* base) {
  CannyWs w{};
  camo_abi::Carver c(base);
  w.grad = c.take<float>(3 * npix);
  w.cls = c.take<unsigned char>(npix);
  w.label = c.take<int>(npix);
  w.flag = c.take<unsigned char>(npix);
  w.bytes = c.bytes();
  return w;
}

int launch_canny_gradients(const float* images, int N, int H, int W, const CannyTaps& taps, float* grad, hipStream_t stream) {
  const int S = T2 + 2 * taps.radius;
  const size_t lds = ((size_t)S * S + (size_t)S * T2 + T2 * T2 + 2 * T2) * sizeof(float);
  hipLaunchKernelGGL(canny_gradient_kernel, dim3((W + T - 1) / T, (H + T - 1) / T, N), dim3(NT), lds, stream, images, H, W, taps, grad);
  return (int)hipGetLastError();
}

int launch_canny_hysteresis(const float* grad, const unsigned char* cls_in, float low, float high, int N, int H, int W, const CannyWs& ws,
                            unsigned char* edges, hipStream_t stream) {
  const dim3 tiles((W + T - 1) / T, (H + T - 1) / T, N);
  const long long total = (long long)N * H * W;
  const unsigned blocks = (unsigned)((total + NT - 1) / NT);
  if (grad)
    hipLaunchKernelGGL(canny_label_tiles_kernel<true>, tiles, dim3(NT), 0, stream, grad, nullptr, ws.cls, low, high, H, W, ws.label, ws.flag);
  else
    hipLaunchKernelGGL(canny_label_tiles_kernel<false>, tiles, dim3(NT), 0, stream, nullptr, cls_in, nullptr, low, high, H, W, ws.label, ws.flag);
  hipLaunchKernelGGL(canny_join_tiles_kernel, dim3(blocks), dim3(NT), 0, stream, ws.label, N, H, W);
  hipLaunchKernelGGL(canny_flag_kernel, dim3(blocks), dim3(NT), 0, stream, ws.label, grad ? ws.cls : cls_in, ws.flag, total);
  hipLaunchKernelGGL(canny_emit_kernel, dim3(blocks), dim3(NT), 0, stream, ws.label, ws.flag, edges, total);
  return (int)hipGetLastError();
}
