// Instance splitter (include/camo_split.h): the components of a label map divided at their necks -- the exact squared
// distance to the background, the cores above a fraction of each id's largest distance, and every pixel of an id with two cores or
// more to the core of its own id with the nearest core pixel.  Every grid covers the whole batch; the launches do not depend on N
// or on the content.
//
//   column .. rank   the ten launches both growth rules run, and their kernels: split_inl.h
//   sites    per (slot, image) and column: the nearest site row of every pixel, a tie to the smaller row
//   nearest  per (slot, image) one block per row: a pixel of the slot's id takes the site of smallest (distance, y', x') and
//            writes that core's id to out
//   table    the rows of the table from out (inst_emit_inl.h)
//
// The image's per-id arrays hold CAMO_IM_MAX_IDS + 1 entries; a label outside 0 .. CAMO_IM_MAX_IDS reads as 0 in every kernel.
// Integer atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "split_inl.h"

namespace {

// grid (ceil(W / COL_X), max_split, images): a site of the slot is a pixel of its id in a kept core.  Per column the nearest site
// row, a tie to the smaller row; -1 where the column has none.
__global__ __launch_bounds__(NT) void split_sites_kernel(const int* __restrict__ labels, const int* __restrict__ par, const int* __restrict__ area, int H,
                                                         int W, int min_core, const int* __restrict__ slot_id, short* __restrict__ site) {
  const int s = blockIdx.y, n = blockIdx.z, x = blockIdx.x * COL_X + threadIdx.x % COL_X;
  const int id = slot_id[(size_t)n * SLOTS + s];
  if (id == 0) return;                                             // (the whole block)
  const size_t img = (size_t)n * H * W + min(x, W - 1);
  const auto hit = [&](int y) {
    const size_t p = img + (size_t)y * W;
    if (labels[p] != id) return false;
    const int r = par[p];
    return r >= 0 && area[r] >= min_core;
  };
  column_nearest(H, W, x < W, hit, site + ((size_t)n * gridDim.y + s) * H * W + min(x, W - 1));
}

// grid (H, max_split, images): a block takes one row of one slot and leaves when the row has no pixel of the slot's id.  Such a
// pixel minimises ((x - x')^2 + (y - y'(x'))^2, y', x') over the columns x', outwards from its own for as long as dx^2 alone does
// not exceed the best (an equal distance may still win the tie), and writes the id of the core that holds the site.
__global__ __launch_bounds__(NT) void split_nearest_kernel(const int* __restrict__ labels, const int* __restrict__ par, const int* __restrict__ rid, int H,
                                                           int W, const int* __restrict__ slot_id, const short* __restrict__ site, int* __restrict__ out) {
  __shared__ int row[SIDE];
  const int y = blockIdx.x, s = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
  const int id = slot_id[(size_t)n * SLOTS + s];
  if (id == 0) return;                                             // (the whole block)
  const size_t base = (size_t)n * H * W, at = base + (size_t)y * W;
  const int* lab = labels + at;
  int mine = 0;
  for (int x = tid; x < W; x += NT) mine |= lab[x] == id;
  if (!__syncthreads_or(mine)) return;
  const short* sr = site + ((size_t)n * gridDim.y + s) * H * W + (size_t)y * W;
  for (int x = tid; x < W; x += NT) row[x] = sr[x];
  __syncthreads();
  for (int x = tid; x < W; x += NT) {
    if (lab[x] != id) continue;
    int best = FAR, by = -1, bx = -1;
    int r = row[x];
    if (r >= 0) { best = (y - r) * (y - r); by = r; bx = x; }
    for (int dx = 1; (long long)dx * dx <= best && (dx <= x || x + dx < W); ++dx) {
      if (dx <= x && (r = row[x - dx]) >= 0) {
        const int c = dx * dx + (y - r) * (y - r);
        if (c < best || (c == best && (r < by || (r == by && x - dx < bx)))) { best = c; by = r; bx = x - dx; }
      }
      if (x + dx < W && (r = row[x + dx]) >= 0) {
        const int c = dx * dx + (y - r) * (y - r);
        if (c < best || (c == best && (r < by || (r == by && x + dx < bx)))) { best = c; by = r; bx = x + dx; }
      }
    }
    out[at + x] = by >= 0 ? rid[par[base + (size_t)by * W + bx]] : 0;      // (a split id has a site)
  }
}

}  // namespace

SplitWs split_carve(int N, int H, int W, int max_split, void* base, bool sites) {
  SplitWs w{};
  camo_abi::Carver c(base);
  const size_t npix = (size_t)N * H * W, chunks = ((size_t)H * W + CHUNK - 1) / CHUNK;
  w.d2 = c.take<int>(npix);
  w.par = c.take<int>(npix);
  w.area = c.take<int>(npix);
  w.rid = c.take<int>(npix);
  w.site = sites ? c.take<short>(npix * max_split) : nullptr;
  w.chunk = c.take<int>((size_t)N * max_split * chunks);
  w.m2 = c.take<int>((size_t)N * PAD);
  w.ncore = c.take<int>((size_t)N * PAD);
  w.parts = c.take<int>((size_t)N * PAD);
  w.first = c.take<int>((size_t)N * PAD);
  w.slot_of = c.take<int>((size_t)N * PAD);
  w.slot_id = c.take<int>((size_t)N * SLOTS);
  w.dropped = c.take<int>((size_t)N);
  w.bytes = c.bytes();
  return w;
}

int launch_split(const int* labels, const float* pred, long long stride, int N, int H, int W, int num, int den, int min_core, int max_split,
                 int max_instances, const SplitWs& ws, int* out, long long* table, int* counts, hipStream_t stream) {
  const long long total = (long long)N * H * W;
  const int chunks = (int)(((long long)H * W + CHUNK - 1) / CHUNK), cols = (W + COL_X - 1) / COL_X;
  const dim3 raster(chunks, N);
  const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
  const long long tiles = (long long)tiles_x * tiles_y;
  // at most 2^32 - 1 threads in a grid: beyond that a block takes several images
  const int tile_rows = (int)std::min<long long>(N, ((1ll << 32) - 1) / (tiles * NT));
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table);
  hipLaunchKernelGGL(split_column_kernel, dim3(cols, N), dim3(NT), 0, stream, labels, H, W, ws.d2, ws.m2, ws.ncore, ws.dropped);
  hipLaunchKernelGGL(split_d2_kernel, dim3(H, N), dim3(NT), 0, stream, labels, H, W, ws.d2, ws.m2);
  hipLaunchKernelGGL(split_core_tiles_kernel, dim3((unsigned)tiles, (unsigned)tile_rows), dim3(NT), 0, stream, labels, ws.d2, ws.m2, (long long)num * num,
                     (long long)den * den, N, H, W, tiles_x, ws.par, ws.area);
  hipLaunchKernelGGL(split_join_kernel, dim3(blocks_of(total)), dim3(NT), 0, stream, labels, ws.par, N, H, W);
  hipLaunchKernelGGL(split_flatten_kernel, raster, dim3(NT), 0, stream, ws.par, ws.area, H, W);
  hipLaunchKernelGGL(split_cores_kernel, raster, dim3(NT), 0, stream, labels, ws.par, ws.area, H, W, min_core, ws.ncore, ws.dropped);
  hipLaunchKernelGGL(split_ids_kernel, dim3(N), dim3(NT), 0, stream, ws.m2, ws.ncore, max_split, ws.parts, ws.first, ws.slot_of, ws.slot_id, ws.dropped,
                     counts);
  hipLaunchKernelGGL(split_count_kernel, raster, dim3(NT), 0, stream, labels, ws.par, ws.area, H, W, min_core, max_split, ws.slot_of, ws.chunk);
  hipLaunchKernelGGL(split_scan_kernel, dim3(max_split, N), dim3(NT), 0, stream, ws.chunk, chunks);
  hipLaunchKernelGGL(split_rank_kernel, raster, dim3(NT), 0, stream, labels, ws.par, ws.area, H, W, min_core, max_split, ws.chunk, ws.first, ws.slot_of,
                     ws.slot_id, counts, max_instances, ws.rid, out, tab);
  hipLaunchKernelGGL(split_sites_kernel, dim3(cols, max_split, N), dim3(NT), 0, stream, labels, ws.par, ws.area, H, W, min_core, ws.slot_id, ws.site);
  hipLaunchKernelGGL(split_nearest_kernel, dim3(H, max_split, N), dim3(NT), 0, stream, labels, ws.par, ws.rid, H, W, ws.slot_id, ws.site, out);
  hipLaunchKernelGGL(split_table_kernel, raster, dim3(NT), 0, stream, pred, stride, out, H, W, max_instances, tab);
  return (int)hipGetLastError();
}
