// Node weights of the structure loss on the painted mask (include/camo_rg_pixel_loss.h): for every node of a
// block-diagonal batch of region graphs, A = sum q and B = sum q g over its pixels, q = K + gain |S - K g| with S the box sum of the
// ground truth g over a (2 r + 1)^2 window.  TWO launches whatever N is; every grid covers the whole batch.
//
//   clear      zero node_w [n_nodes, 2]
//   accumulate one block per 32 x 32 tile of one image (the shape of rgtg_accumulate_kernel).  The tile's ground truth with a halo of
//              r is staged in LDS as bytes 0 / 1 (outside the image: 0, the zero padding of the definition), at most 94 x 94 of them.
//              The box sum is separable: row sums of 2 r + 1 bytes for the 32 columns of every halo row (at most 63: a byte again),
//              then per pixel a column sum of 2 r + 1 of those, all LDS reads.  q and q g go into the LDS slot table keyed by the
//              node (label_slot): a tile's sum is at most 1024 * 17 * 63^2 < 2^32, so one or two 32-bit integer LDS atomics per
//              pixel; then one 64-bit integer global atomic per occupied slot and non-zero quantity.  A node that finds the table
//              full adds to global memory directly: either way the same integers reach the same sum.
//
// Blocks meet only in relaxed agent-scope integer atomics on node_w, whose results nobody reads before the launch ends.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "label_inl.h"
#include "rg_targets.h"
#include "rg_pixel_loss.h"

namespace {

constexpr int T = RGTG_TILE, NT = 256, PPT = T * T / NT, SLOTS = RGTG_SLOTS, LWMAX = T + 2 * RGPL_MAX_RADIUS;
constexpr long long KMAX = (2 * RGPL_MAX_RADIUS + 1) * (2 * RGPL_MAX_RADIUS + 1);
static_assert(2 * RGPL_MAX_RADIUS + 1 < 256, "a row sum is a byte");
static_assert((long long)T * T * KMAX * (1 + RGPL_MAX_GAIN) < (1ll << 32), "a tile's sum of q is a 32-bit word");

__global__ __launch_bounds__(NT) void rgpl_clear_kernel(long long* __restrict__ node_w, size_t total) {
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < total; k += stride) node_w[k] = 0;
}

__global__ __launch_bounds__(NT) void rgpl_accumulate_kernel(const int* __restrict__ seg, const int* __restrict__ rmap,
                                                             const int* __restrict__ node_off, const unsigned char* __restrict__ gt_mask,
                                                             int H, int W, int tiles_x, int tiles_y, int label_bound, int n_nodes, int r, int gain,
                                                             long long* node_w) {
  __shared__ unsigned char g[LWMAX * LWMAX];      // [lw][lw], lw = T + 2 r: the tile's ground truth and its halo
  __shared__ unsigned char rs[LWMAX * T];         // [lw][T]: rs[ly][lx] = g[ly][lx] + .. + g[ly][lx + 2 r]
  __shared__ int keys[SLOTS];
  __shared__ unsigned int tab[SLOTS][2];
  // (one grid dimension: N and the tile rows of a tall image may both pass 65535)
  const int tid = threadIdx.x, per_image = tiles_x * tiles_y, n = blockIdx.x / per_image, tile = blockIdx.x - n * per_image;
  const int ty0 = tile / tiles_x * T, tx0 = tile % tiles_x * T;
  const int lw = T + 2 * r, win = 2 * r + 1, K = win * win;
  const size_t HW = (size_t)H * W, base = (size_t)n * HW;
  for (int i = tid; i < SLOTS; i += NT) { keys[i] = -1; tab[i][0] = 0u; tab[i][1] = 0u; }
  for (int i = tid; i < lw * lw; i += NT) {
    const int ly = i / lw, lx = i - ly * lw, y = ty0 - r + ly, x = tx0 - r + lx;
    g[i] = (y >= 0 && y < H && x >= 0 && x < W) ? (unsigned char)(gt_mask[base + (size_t)y * W + x] > 127) : (unsigned char)0;
  }
  __syncthreads();
  for (int i = tid; i < lw * T; i += NT) {
    const int ly = i / T, lx = i - ly * T;
    const unsigned char* row = g + ly * lw + lx;
    int s = 0;
    for (int d = 0; d < win; ++d) s += row[d];
    rs[i] = (unsigned char)s;
  }
  __syncthreads();
  const long long first = node_off[n];
  const int* rmapn = rmap + (size_t)n * label_bound;
  for (int j = 0; j < PPT; ++j) {
    const int t = tid + j * NT, ly = t / T, lx = t - ly * T, y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    const int s = seg[base + (size_t)y * W + x];
    if ((unsigned)s >= (unsigned)label_bound) continue;
    const int reg = rmapn[s];
    if (reg < 0) continue;
    const long long row = first + reg;
    if (row < 0 || row >= n_nodes) continue;
    const int v = (int)row;
    const unsigned char* col = rs + ly * T + lx;
    int S = 0;
    for (int d = 0; d < win; ++d) S += col[d * T];
    const int m = g[(ly + r) * lw + lx + r];
    const unsigned q = (unsigned)(K + gain * abs(S - K * m));
    const int slot = label_slot<SLOTS>(keys, v);
    if (slot >= 0) {
      atomicAdd(&tab[slot][0], q);
      if (m) atomicAdd(&tab[slot][1], q);
    } else {
      unsigned long long* a = reinterpret_cast<unsigned long long*>(node_w) + (size_t)v * 2;
      atomicAdd(a, (unsigned long long)q);
      if (m) atomicAdd(a + 1, (unsigned long long)q);
    }
  }
  __syncthreads();
  for (int i = tid; i < SLOTS * 2; i += NT) {
    const int k = keys[i >> 1];
    if (k < 0) continue;
    const unsigned val = tab[i >> 1][i & 1];
    if (val) atomicAdd(reinterpret_cast<unsigned long long*>(node_w) + (size_t)k * 2 + (i & 1), (unsigned long long)val);
  }
}

}  // namespace

int launch_rg_pixel_weights(const int* segments, const int* region_map, const int* node_off, const unsigned char* gt_mask, int N, int H, int W,
                            int label_bound, int n_nodes, int radius, int gain, long long* node_w, hipStream_t stream) {
  const size_t total = (size_t)n_nodes * 2;
  const unsigned clear_blocks = (unsigned)std::min<size_t>((total + NT - 1) / NT, 2048);
  hipLaunchKernelGGL(rgpl_clear_kernel, dim3(clear_blocks), dim3(NT), 0, stream, node_w, total);
  const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;               // N tiles_x tiles_y <= N H W <= 2^27
  hipLaunchKernelGGL(rgpl_accumulate_kernel, dim3((unsigned)N * tiles_x * tiles_y), dim3(NT), 0, stream, segments, region_map, node_off,
                     gt_mask, H, W, tiles_x, tiles_y, label_bound, n_nodes, radius, gain, node_w);
  return (int)hipGetLastError();
}
