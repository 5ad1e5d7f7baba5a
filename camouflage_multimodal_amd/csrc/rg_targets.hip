// Node targets from ground-truth masks (include/camo_rg_targets.h): for every node of a block-diagonal batch of region graphs, how
// many of its pixels are positive in the mask, the instance mask and the edge map, and the three targets camo_rg_loss_backward
// takes.  THREE launches whatever N is; every grid covers the whole batch.
//
//   clear      zero counts [n_nodes, 4]
//   accumulate one block per 32 x 32 tile of one image (the shape of rgb_accumulate_kernel).  The tile's mask bytes with a halo of 1
//              are staged in LDS as positive / not positive / outside the image, so the four neighbour reads of the boundary rule are
//              LDS reads.  Per-node sums go into an LDS hash table keyed by the node index: a tile holds at most 1024 pixels, so
//              two 16-bit fields share a word (pixels | mask << 16, instance | edge << 16) and a pixel costs one or two 32-bit
//              integer LDS atomics.  Then one 32-bit integer global atomic per occupied slot and non-zero quantity.  A node that finds
//              the table full adds to global memory directly: either way the same integers reach the same sum.
//   finalize   one lane per node: the comparisons of the header in 64-bit integers.
//
// Blocks meet only in relaxed agent-scope integer atomics on counts, whose results nobody reads before the launch ends; finalize
// reads them in stream order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "label_inl.h"
#include "rg_targets.h"

namespace {

constexpr int T = RGTG_TILE, NT = 256, PPT = T * T / NT, LW = T + 2, SLOTS = RGTG_SLOTS;
static_assert(T * T < (1 << 16), "two counts of a tile share a 32-bit word");
enum : unsigned char { NEG = 0, POS = 1, OUTSIDE = 2 };

__global__ __launch_bounds__(NT) void rgtg_clear_kernel(int* __restrict__ counts, size_t total) {
  const size_t stride = (size_t)gridDim.x * NT;
  for (size_t k = (size_t)blockIdx.x * NT + threadIdx.x; k < total; k += stride) counts[k] = 0;
}

__global__ __launch_bounds__(NT) void rgtg_accumulate_kernel(const int* __restrict__ seg, const int* __restrict__ rmap,
                                                             const int* __restrict__ node_off, const unsigned char* __restrict__ gt_mask,
                                                             const unsigned char* __restrict__ gt_inst,
                                                             const unsigned char* __restrict__ gt_edge, int H, int W, int tiles_x,
                                                             int tiles_y, int label_bound, int n_nodes, int* counts) {
  __shared__ unsigned char pos[LW * LW];
  __shared__ int keys[SLOTS];
  __shared__ unsigned int tab[SLOTS][2];
  // (one grid dimension: N and the tile rows of a tall image may both pass 65535)
  const int tid = threadIdx.x, per_image = tiles_x * tiles_y, n = blockIdx.x / per_image, tile = blockIdx.x - n * per_image;
  const int ty0 = tile / tiles_x * T, tx0 = tile % tiles_x * T;
  const size_t HW = (size_t)H * W, base = (size_t)n * HW;
  for (int i = tid; i < SLOTS; i += NT) { keys[i] = -1; tab[i][0] = 0u; tab[i][1] = 0u; }
  for (int i = tid; i < LW * LW; i += NT) {
    const int ly = i / LW, lx = i - ly * LW, y = ty0 - 1 + ly, x = tx0 - 1 + lx;
    unsigned char c = OUTSIDE;
    if (y >= 0 && y < H && x >= 0 && x < W) c = gt_mask[base + (size_t)y * W + x] > 127 ? POS : NEG;
    pos[i] = c;
  }
  __syncthreads();
  const long long first = node_off[n];
  const int* rmapn = rmap + (size_t)n * label_bound;
  for (int j = 0; j < PPT; ++j) {
    const int t = tid + j * NT, ly = t / T, lx = t - ly * T, y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    const size_t p = base + (size_t)y * W + x;
    const int s = seg[p];
    if ((unsigned)s >= (unsigned)label_bound) continue;
    const int r = rmapn[s];
    if (r < 0) continue;
    const long long row = first + r;
    if (row < 0 || row >= n_nodes) continue;
    const int v = (int)row;
    const unsigned char* c = pos + (ly + 1) * LW + (lx + 1);
    const unsigned m = c[0] == POS;
    const unsigned in = gt_inst ? (unsigned)(gt_inst[p] > 127) : m;
    unsigned e;
    if (gt_edge) e = gt_edge[p] > 127;
    else e = m && (c[-LW] == NEG || c[LW] == NEG || c[-1] == NEG || c[1] == NEG);      // (OUTSIDE is no neighbour)
    const unsigned w0 = 1u | (m << 16), w1 = in | (e << 16);
    const int slot = label_slot<SLOTS>(keys, v);
    if (slot >= 0) {
      atomicAdd(&tab[slot][0], w0);
      if (w1) atomicAdd(&tab[slot][1], w1);
    } else {
      int* a = counts + (size_t)v * 4;
      atomicAdd(a, 1);
      if (m) atomicAdd(a + 1, 1);
      if (in) atomicAdd(a + 2, 1);
      if (e) atomicAdd(a + 3, 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < SLOTS * 4; i += NT) {
    const int k = keys[i >> 2], q = i & 3;
    if (k < 0) continue;
    const unsigned w = tab[i >> 2][q >> 1];
    const int val = (int)((q & 1) ? (w >> 16) : (w & 0xFFFFu));
    if (val) atomicAdd(counts + (size_t)k * 4 + q, val);
  }
}

__device__ __forceinline__ int rgtg_vote(long long pos, long long pix, long long band) {
  if (1000ll * pos > (500ll + band) * pix) return 1;
  if (1000ll * pos <= (500ll - band) * pix) return 0;
  return -1;
}

__global__ __launch_bounds__(NT) void rgtg_finalize_kernel(const int* __restrict__ counts, int n_nodes, int band, int edge_min,
                                                           int* __restrict__ mask_t, int* __restrict__ inst_t, float* __restrict__ edge_t) {
  const int v = blockIdx.x * NT + threadIdx.x;
  if (v >= n_nodes) return;
  const int* c = counts + (size_t)v * 4;
  const int pix = c[0];
  if (pix == 0) { mask_t[v] = -1; inst_t[v] = -1; edge_t[v] = -1.0f; return; }
  mask_t[v] = rgtg_vote(c[1], pix, band);
  inst_t[v] = rgtg_vote(c[2], pix, band);
  edge_t[v] = c[3] >= edge_min ? 1.0f : 0.0f;
}

}  // namespace

int launch_rg_node_targets(const int* segments, const int* region_map, const int* node_off, const unsigned char* gt_mask,
                           const unsigned char* gt_instance, const unsigned char* gt_edge, int N, int H, int W, int label_bound, int n_nodes,
                           int band_permille, int edge_min_pixels, int* counts, int* mask_t, int* inst_t, float* edge_t, hipStream_t stream) {
  const size_t total = (size_t)n_nodes * 4;
  const unsigned clear_blocks = (unsigned)std::min<size_t>((total + NT - 1) / NT, 2048);
  hipLaunchKernelGGL(rgtg_clear_kernel, dim3(clear_blocks), dim3(NT), 0, stream, counts, total);
  const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;               // N tiles_x tiles_y <= N H W <= 2^27
  hipLaunchKernelGGL(rgtg_accumulate_kernel, dim3((unsigned)N * tiles_x * tiles_y), dim3(NT), 0, stream, segments, region_map, node_off,
                     gt_mask, gt_instance, gt_edge, H, W, tiles_x, tiles_y, label_bound, n_nodes, counts);
  hipLaunchKernelGGL(rgtg_finalize_kernel, dim3((n_nodes + NT - 1) / NT), dim3(NT), 0, stream, counts, n_nodes, band_permille,
                     edge_min_pixels, mask_t, inst_t, edge_t);
  return (int)hipGetLastError();
}
