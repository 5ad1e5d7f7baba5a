// Geodesic growth for the instance splitter (include/camo_split_geo.h): after the ten launches that split.hip runs
// too (split_inl.h), every pixel of a split id goes to the kept core of its id that the cheapest path INSIDE the id reaches, links
// to the 8 neighbours at 5 (straight) and 7 (diagonal), a tie to the smaller new id.  The launches are a function of `rounds` alone.
//
//   init     one block per 32 x 32 tile: key = (new id, slot) at path cost 0 on the kept core pixels of the split ids, (slot) at a cost
//            no path has on their other pixels, 0 elsewhere.  The tile is flagged for round 0 when it or its one-pixel halo holds
//            such a core pixel (a core that ends on a tile border never changes, so it could not flag the neighbour later)
//   grow     one block per tile, a thread a pixel, `rounds` launches.  A tile whose flag of this round is clear returns.  Otherwise its
//            34 x 34 keys are loaded into LDS and relaxed by Jacobi sweeps -- every thread reads its neighbours, a barrier, every thread
//            writes what went down and says so in an LDS flag, a barrier -- until nothing changes, at most SPLIT_GEO_SWEEPS times; the
//            interior keys that went down are stored, the neighbours that touch a changed pixel of the outer ring are flagged for
//            the next round, and the tile itself when it was still changing at the bound
//   finish   out = the new id in the key, the id's first part where no core reached, first[id] + 1 / 0 off the split ids as the rank
//            launch wrote; the table's rows cleared again (a resume adds to them a second time); an image's first block counts the
//            tiles flagged for the round that was not run into pending[n] and moves those flags to the even buffer, where a resume
//            starts
//   table    split_inl.h
//
// Keys are compared as whole 64-bit integers: inside one slot the low four bits are equal, so the order is (path cost, new id).  The
// relaxation key(p) = min(key(p), key(q) + (w << 32)) over the neighbours q of p's slot keeps that order, and only ever lowers a key;
// the state with no flag set is its one fixed point, whatever each block happened to read on the way.  A block
// writes the keys of its own tile only, a flag only ever to 1 from other tiles, and waits for nobody.  No atomics on memory; the
// ring mask is an LDS atomicOr.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "split_inl.h"
#include "../../include/camo_split_geo.h"

namespace {

using Key = unsigned long long;
constexpr int HALO = T + 2, LS = HALO;             // the LDS tile with its ring.  A half wave reads 32 consecutive keys of one row: 64 banks
constexpr int SWEEPS = SPLIT_GEO_SWEEPS, GNT = T * T;
constexpr unsigned NO_LINK = 0x7fffffffu;          // FAR_G + NO_LINK < 2^32: no carry out of the key
constexpr Key FAR_G = 1ull << 30;                  // a path cost no path has (7 * 2048^2 < 2^25).  A key that holds it never changes:
                                                   // what a neighbour offers is its own key plus a link, and that is larger
constexpr int SELF = 4;                            // bit (dy + 1) * 3 + (dx + 1) of the ring mask: the tile itself
static_assert(T == SPLIT_GEO_TILE && T == CAMO_SPLIT_GEO_TILE && GNT <= 1024 && 64 / T == 2 && T % 2 == 0, "a wave takes two whole rows of a tile");
static_assert(7ll * SIDE * SIDE < (1ll << 25) && SLOTS < 15 && (long long)SIDE * SIDE < (1ll << 27), "cost, slot and new id fit the key");

__device__ __forceinline__ int key_slot(Key k) { return (int)(k & 15); }      // slot + 1, 0: not a pixel of a split id

// grid (tiles of an image, images; an image loop when the grid would be too large)
__global__ __launch_bounds__(NT) void split_geo_init_kernel(const int* __restrict__ labels, const int* __restrict__ par, const int* __restrict__ area,
                                                            const int* __restrict__ rid, const int* __restrict__ slot_of, int min_core, int N, int H,
                                                            int W, int tiles_x, Key* __restrict__ key, int* __restrict__ flag0, int* __restrict__ flag1) {
  const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * T - 1, x0 = tx * T - 1;
  const size_t HW = (size_t)H * W;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const size_t base = (size_t)n * HW;
    int seeds = 0;
    for (int l = tid; l < HALO * HALO; l += NT) {
      const int hy = l / HALO, hx = l - hy * HALO, y = y0 + hy, x = x0 + hx;
      if (y < 0 || y >= H || x < 0 || x >= W) continue;
      const size_t p = base + (size_t)y * W + x;
      const int id = split_id(labels[p]);
      const int s = id ? slot_of[(size_t)n * PAD + id] : -1;
      Key k = 0;
      if (s >= 0) {
        const int r = par[p];
        const bool kept = r >= 0 && area[r] >= min_core;
        k = kept ? ((Key)rid[r] << 4) | (Key)(s + 1) : (FAR_G << 32) | (Key)(s + 1);
        seeds |= kept;
      }
      if (hy >= 1 && hy <= T && hx >= 1 && hx <= T) key[p] = k;
    }
    seeds = __syncthreads_or(seeds);
    if (tid == 0) {
      flag0[(size_t)n * gridDim.x + blockIdx.x] = seeds != 0;
      flag1[(size_t)n * gridDim.x + blockIdx.x] = 0;
    }
  }
}

// grid as init, GNT threads: one a pixel of the tile.  cur: this round's flags, next: the next round's (all clear on entry: every
// tile that ran cleared its own).  A sweep costs a wave its instructions whatever the other waves do, so a thread holds one pixel and
// its eight link weights in registers (a neighbour that is not linked weighs NO_LINK: what it offers is above every key), and a
// wave -- two tile rows -- sits a sweep out when no key of its rows or the two beside them went down in the sweep before.
__global__ __launch_bounds__(GNT) void split_geo_grow_kernel(Key* key, int* cur, int* next, int N, int H, int W, int tiles_x, int tiles_y) {
  __shared__ Key k[HALO * LS];
  __shared__ int went[2][HALO];                                                   // went[s & 1][row + 1]: a key of the tile row went down in sweep s
  __shared__ int moved[2], ring;                                                  // moved[s & 1]: a key went down in sweep s
  const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * T - 1, x0 = tx * T - 1;
  const int ly = tid / T, lx = tid % T, at = (ly + 1) * LS + lx + 1, rows = tid / 64 * (64 / T);      // rows: the first tile row of the thread's wave
  const size_t HW = (size_t)H * W;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    int* mine = cur + (size_t)n * gridDim.x + blockIdx.x;
    if (*mine == 0) continue;                                                     // (the whole block: nobody writes it before the barrier below)
    const size_t base = (size_t)n * HW;
    for (int l = tid; l < HALO * HALO; l += GNT) {
      const int hy = l / HALO, hx = l - hy * HALO, y = y0 + hy, x = x0 + hx;
      k[hy * LS + hx] = (y >= 0 && y < H && x >= 0 && x < W) ? key[base + (size_t)y * W + x] : 0;
    }
    if (tid < HALO) { went[0][tid] = 0; went[1][tid] = tid >= 1 && tid <= T; }    // (sweep 0 reads went[1]: every row counts as changed)
    if (tid == 0) { ring = 0; moved[0] = 0; moved[1] = 1; }
    __syncthreads();
    if (tid == 0) *mine = 0;
    const Key was = k[at];
    Key now = was;
    unsigned w[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int r = (b < 4 ? b : b + 1) / 3, c = (b < 4 ? b : b + 1) % 3;          // (the eight cells of the 3 x 3 around the pixel)
      const bool linked = key_slot(was) != 0 && key_slot(k[at + (r - 1) * LS + c - 1]) == key_slot(was);
      w[b] = linked ? (r == 1 || c == 1 ? 5u : 7u) : NO_LINK;
    }
    int sweep = 0;
    for (; sweep < SWEEPS; ++sweep) {
      const int* before = went[(sweep + 1) & 1];
      if (moved[(sweep + 1) & 1] == 0) break;                                     // (the whole block: written before the last barrier)
      Key best = now;
      if (before[rows] | before[rows + 1] | before[rows + 2] | before[rows + 3]) {      // (the whole wave)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const int r = (b < 4 ? b : b + 1) / 3, c = (b < 4 ? b : b + 1) % 3;
          const Key cand = k[at + (r - 1) * LS + c - 1] + ((Key)w[b] << 32);
          if (cand < best) best = cand;
        }
      }
      __syncthreads();                                                            // every read of this sweep is done
      if (tid < HALO) went[(sweep + 1) & 1][tid] = 0;
      if (tid == 0) moved[(sweep + 1) & 1] = 0;
      if (best < now) { now = best; k[at] = best; went[sweep & 1][ly + 1] = 1; moved[sweep & 1] = 1; }
      __syncthreads();
    }
    int m = sweep == SWEEPS && moved[(sweep + 1) & 1] ? 1 << SELF : 0;            // the last sweep still lowered a key
    if (now < was) {                                                              // (only a pixel of a split id goes down: it is inside the image)
      key[base + (size_t)(y0 + 1 + ly) * W + x0 + 1 + lx] = now;
      const int dy0 = ly == 0 ? -1 : 0, dy1 = ly == T - 1 ? 1 : 0, dx0 = lx == 0 ? -1 : 0, dx1 = lx == T - 1 ? 1 : 0;
      for (int dy = dy0; dy <= dy1; ++dy)
        for (int dx = dx0; dx <= dx1; ++dx)
          if (dy | dx) m |= 1 << ((dy + 1) * 3 + dx + 1);
    }
    if (m) atomicOr(&ring, m);
    __syncthreads();
    if (tid < 9 && (ring >> tid & 1)) {
      const int v = ty + tid / 3 - 1, u = tx + tid % 3 - 1;
      if (v >= 0 && v < tiles_y && u >= 0 && u < tiles_x) next[(size_t)n * gridDim.x + v * tiles_x + u] = 1;
    }
    __syncthreads();                                                              // k, went and ring are reused by the next image
  }
}

// grid (chunks, images).  pend: the flags of the round after the last one run; even: flag[0]
__global__ __launch_bounds__(NT) void split_geo_finish_kernel(const int* __restrict__ labels, const Key* __restrict__ key, const int* __restrict__ first,
                                                              const int* __restrict__ counts, int H, int W, int max_instances, int tiles,
                                                              int* __restrict__ out, unsigned long long* __restrict__ table, int* pend, int* even,
                                                              int* __restrict__ pending) {
  __shared__ int wsum[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  emit_clear_rows<NT>(table + (size_t)n * max_instances * 8, counts[4 * n], max_instances);
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    if (q >= HW) continue;
    const int id = split_id(labels[base + q]);
    const Key kv = key[base + q];
    const bool reached = key_slot(kv) != 0 && (kv >> 32) < FAR_G;
    out[base + q] = !id ? 0 : reached ? (int)((unsigned)kv >> 4) : first[(size_t)n * PAD + id] + 1;
  }
  if (blockIdx.x != 0) return;                                                    // (the whole block)
  int left = 0;
  for (int t = tid; t < tiles; t += NT) {
    const int f = pend[(size_t)n * tiles + t];
    left += f != 0;
    if (pend != even) { even[(size_t)n * tiles + t] = f; pend[(size_t)n * tiles + t] = 0; }
  }
  left = wave_sum_int(left);
  if ((tid & 63) == 0) wsum[tid >> 6] = left;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < NT / 64; ++w) total += wsum[w];
    pending[n] = total;
  }
}

}  // namespace

SplitGeoWs split_geo_carve(int N, int H, int W, int max_split, void* base) {
  SplitGeoWs w{};
  w.s = split_carve(N, H, W, max_split, base, false);
  camo_abi::Carver c(base, w.s.bytes);
  const size_t tiles = (size_t)((W + T - 1) / T) * ((H + T - 1) / T);
  w.key = c.take<Key>((size_t)N * H * W);
  w.flag[0] = c.take<int>((size_t)N * tiles);
  w.flag[1] = c.take<int>((size_t)N * tiles);
  w.bytes = c.bytes();
  return w;
}

int launch_split_geo_resume(const int* labels, const float* pred, long long stride, int N, int H, int W, int max_instances, int rounds,
                            const SplitGeoWs& ws, int* out, long long* table, const int* counts, int* pending, hipStream_t stream) {
  const int chunks = (int)(((long long)H * W + CHUNK - 1) / CHUNK), tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
  const long long tiles = (long long)tiles_x * tiles_y;
  // at most 2^32 - 1 threads in a grid: beyond that a block takes several images
  const dim3 raster(chunks, N), tiled((unsigned)tiles, (unsigned)std::min<long long>(N, ((1ll << 32) - 1) / (tiles * GNT)));
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table);
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(split_geo_grow_kernel, tiled, dim3(GNT), 0, stream, ws.key, ws.flag[r & 1], ws.flag[(r + 1) & 1], N, H, W, tiles_x, tiles_y);
  hipLaunchKernelGGL(split_geo_finish_kernel, raster, dim3(NT), 0, stream, labels, ws.key, ws.s.first, counts, H, W, max_instances, (int)tiles, out, tab,
                     ws.flag[rounds & 1], ws.flag[0], pending);
  hipLaunchKernelGGL(split_table_kernel, raster, dim3(NT), 0, stream, pred, stride, out, H, W, max_instances, tab);
  return (int)hipGetLastError();
}

int launch_split_geo(const int* labels, const float* pred, long long stride, int N, int H, int W, int num, int den, int min_core, int max_split,
                     int max_instances, int rounds, const SplitGeoWs& ws, int* out, long long* table, int* counts, int* pending, hipStream_t stream) {
  const SplitWs& s = ws.s;
  const long long total = (long long)N * H * W;
  const int chunks = (int)(((long long)H * W + CHUNK - 1) / CHUNK), cols = (W + COL_X - 1) / COL_X;
  const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
  const long long tiles = (long long)tiles_x * tiles_y;
  // at most 2^32 - 1 threads in a grid: beyond that a block takes several images
  const dim3 raster(chunks, N), tiled((unsigned)tiles, (unsigned)std::min<long long>(N, ((1ll << 32) - 1) / (tiles * NT)));
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table);
  hipLaunchKernelGGL(split_column_kernel, dim3(cols, N), dim3(NT), 0, stream, labels, H, W, s.d2, s.m2, s.ncore, s.dropped);
  hipLaunchKernelGGL(split_d2_kernel, dim3(H, N), dim3(NT), 0, stream, labels, H, W, s.d2, s.m2);
  hipLaunchKernelGGL(split_core_tiles_kernel, tiled, dim3(NT), 0, stream, labels, s.d2, s.m2, (long long)num * num, (long long)den * den, N, H, W, tiles_x,
                     s.par, s.area);
  hipLaunchKernelGGL(split_join_kernel, dim3(blocks_of(total)), dim3(NT), 0, stream, labels, s.par, N, H, W);
  hipLaunchKernelGGL(split_flatten_kernel, raster, dim3(NT), 0, stream, s.par, s.area, H, W);
  hipLaunchKernelGGL(split_cores_kernel, raster, dim3(NT), 0, stream, labels, s.par, s.area, H, W, min_core, s.ncore, s.dropped);
  hipLaunchKernelGGL(split_ids_kernel, dim3(N), dim3(NT), 0, stream, s.m2, s.ncore, max_split, s.parts, s.first, s.slot_of, s.slot_id, s.dropped, counts);
  hipLaunchKernelGGL(split_count_kernel, raster, dim3(NT), 0, stream, labels, s.par, s.area, H, W, min_core, max_split, s.slot_of, s.chunk);
  hipLaunchKernelGGL(split_scan_kernel, dim3(max_split, N), dim3(NT), 0, stream, s.chunk, chunks);
  hipLaunchKernelGGL(split_rank_kernel, raster, dim3(NT), 0, stream, labels, s.par, s.area, H, W, min_core, max_split, s.chunk, s.first, s.slot_of,
                     s.slot_id, counts, max_instances, s.rid, out, tab);
  hipLaunchKernelGGL(split_geo_init_kernel, tiled, dim3(NT), 0, stream, labels, s.par, s.area, s.rid, s.slot_of, min_core, N, H, W, tiles_x, ws.key,
                     ws.flag[0], ws.flag[1]);
  return launch_split_geo_resume(labels, pred, stride, N, H, W, max_instances, rounds, ws, out, table, counts, pending, stream);
}
