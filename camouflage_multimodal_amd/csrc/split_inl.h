// The kernels of the instance splitter that both growth rules run (split.hip: the Euclidean cells of include/camo_split.h;
// split_geo.hip: the geodesic cells of include/camo_split_geo.h), stated once as cc_inl.h and label_inl.h state
// theirs: the ten launches from the distance transform to each kept core's new id, and the table over out_labels.  Each file that
// includes this states its own launch list; the kernels have internal linkage.  split_merge.hip (include/camo_split_merge.h, 10u)
// takes the device functions only: column_nearest, row_distance2 and table_rows.
//
//   column   per column the nearest background row of every pixel, 16 columns by 16 row segments a block (column_nearest); the first
//            block of an image clears its per-id arrays
//   d2       one block per image row, the column's rows staged in LDS: D2 in place, and M2 by integer max through an LDS table
//   tiles    one block per 32 x 32 tile: the core pixels and their components in LDS, `same` = equal id (cc_inl.h)
//   join     core pixels on a tile border: cc_inl.h's unions across the borders, same rule
//   flatten  every core pixel finds its root and points at it; area[root] counts it, runs of equal root combined in the wave
//   cores    per id the cores of at least min_core pixels; the smaller ones counted
//   ids      one block per image: the ids with two kept cores ranked (label_compact), the first max_split named as slots, the parts of
//            every id scanned into its first new id (label_scan); counts
//   count    per chunk of 1024 pixels and slot: the slot's kept roots
//   scan     one block per (slot, image): the chunks' exclusive prefix
//   rank     rid[root] = the id's first new id + the kept roots of the id before it; out of everything that is not split; the
//            image's table rows cleared
//   table    the rows of the table from out (inst_emit_inl.h)
//
// The image's per-id arrays hold CAMO_IM_MAX_IDS + 1 entries; a label outside 0 .. CAMO_IM_MAX_IDS reads as 0 in every kernel.
// Integer atomics only.
#pragma once
#include <hip/hip_runtime.h>

#include "cc_inl.h"
#include "common.h"
#include "inst_emit_inl.h"
#include "instances.h"
#include "label_inl.h"
#include "split.h"
#include "../../include/camo_split.h"

namespace {

constexpr int T = INST_TILE, NT = INST_NT, CHUNK = INST_CHUNK, PPT = INST_CHUNK / INST_NT;
constexpr int IDS = SPLIT_IDS, PAD = SPLIT_IDS_PAD, SLOTS = SPLIT_MAX_SLOTS, SIDE = SPLIT_MAX_SIDE;
constexpr int FAR = 0x7fffffff;
static_assert(IDS == CAMO_IM_MAX_IDS + 1 && PAD >= IDS && SLOTS == CAMO_SPLIT_MAX_SPLIT && SIDE == CAMO_SEG_WF_MAX_SIDE, "include/camo_split.h states the limits");
static_assert(T * T % NT == 0 && CHUNK % NT == 0 && NT % 64 == 0 && NT >= EMIT_SLOTS * 8, "whole waves, whole passes");
static_assert(2ll * (SIDE - 1) * (SIDE - 1) + 2 < FAR && (long long)CAMO_SPLIT_MAX_DEN * CAMO_SPLIT_MAX_DEN * 2 * SIDE * SIDE < (1ll << 62), "distances are ints, the core test 64-bit");

__device__ __forceinline__ int split_id(int L) { return (unsigned)L < (unsigned)IDS ? L : 0; }

// The nearest row with hit(y) of every pixel of a column, a tie to the smaller row, -1 where the column has none: out[y * W] for y < H.
// A block's NT threads are COL_X consecutive columns by COL_SEGS segments of consecutive rows, so that a batch of small images
// still fills the device; `mine`: the thread's column is inside the image.  A thread sweeps down its segment (the last hit at or
// above y, -1 when the segment has none yet), the segments' first and last hits meet in LDS, and the sweep up takes the last hit of
// the segments above where its own has none and starts from the first hit of the segments below.  Every thread of the block calls.
constexpr int COL_X = 16, COL_SEGS = NT / COL_X;
template <class Hit, class V>
__device__ __forceinline__ void column_nearest(int H, int W, bool mine, Hit hit, V* __restrict__ out) {
  __shared__ int seg_first[COL_SEGS][COL_X], seg_last[COL_SEGS][COL_X];
  const int c = threadIdx.x % COL_X, seg = threadIdx.x / COL_X, rows = (H + COL_SEGS - 1) / COL_SEGS;
  const int y0 = min(seg * rows, H), y1 = min(y0 + rows, H);
  int first = -1, last = -1;
  if (mine)
    for (int y = y0; y < y1; ++y) {
      if (hit(y)) { if (first < 0) first = y; last = y; }
      out[(size_t)y * W] = (V)last;
    }
  seg_first[seg][c] = first; seg_last[seg][c] = last;
  __syncthreads();
  if (!mine) return;
  int above = -1, below = -1;
  for (int t = 0; t < seg; ++t) above = max(above, seg_last[t][c]);
  for (int t = COL_SEGS - 1; t > seg; --t)
    if (seg_first[t][c] >= 0) below = seg_first[t][c];
  for (int y = y1 - 1; y >= y0; --y) {
    int up = out[(size_t)y * W];
    if (up < 0) up = above;
    if (up == y) below = y;
    out[(size_t)y * W] = (V)(up < 0 ? below : below < 0 ? up : (y - up <= below - y ? up : below));
  }
}

// grid (ceil(W / COL_X), N): per column the nearest background row of every pixel.  An image's first block clears its per-id arrays.
__global__ __launch_bounds__(NT) void split_column_kernel(const int* __restrict__ labels, int H, int W, int* __restrict__ ny, int* __restrict__ m2,
                                                          int* __restrict__ ncore, int* __restrict__ dropped) {
  const int n = blockIdx.y, tid = threadIdx.x, x = blockIdx.x * COL_X + tid % COL_X;
  if (blockIdx.x == 0) {
    for (int i = tid; i < IDS; i += NT) { m2[(size_t)n * PAD + i] = 0; ncore[(size_t)n * PAD + i] = 0; }
    if (tid == 0) dropped[n] = 0;
  }
  const int* g = labels + (size_t)n * H * W + min(x, W - 1);
  column_nearest(H, W, x < W, [&](int y) { return split_id(g[(size_t)y * W]) == 0; }, ny + (size_t)n * H * W + min(x, W - 1));
}

// D2 of the foreground pixel (y, x) from row[]: the nearest background row of every column of the image, as column_nearest leaves
// it, staged in LDS.  The pixel starts from its own column's distance and looks at the columns dx to the left and right for as long
// as dx^2 alone is below the best: nothing farther can be nearer.  -1 when no column has a row to offer: the image has no background.
// (split_d2_kernel, and split_merge.hip's d2 launch)
__device__ __forceinline__ int row_distance2(const int* row, int W, int x, int y) {
  int best = FAR;
  int r = row[x];
  if (r >= 0) best = (y - r) * (y - r);
  for (int dx = 1; dx * dx < best && (dx <= x || x + dx < W); ++dx) {
    if (dx <= x && (r = row[x - dx]) >= 0) best = min(best, dx * dx + (y - r) * (y - r));
    if (x + dx < W && (r = row[x + dx]) >= 0) best = min(best, dx * dx + (y - r) * (y - r));
  }
  return best == FAR ? -1 : best;
}

// grid (H, N): a block takes one row.  The row is overwritten in place with D2 (row_distance2; 0 on background, -1 when the image has
// no background).  top[id] = the row's largest D2 + 2 (so that an id with a pixel is never 0), added to m2 once per block and id.
__global__ __launch_bounds__(NT) void split_d2_kernel(const int* __restrict__ labels, int H, int W, int* __restrict__ d2, int* __restrict__ m2) {
  __shared__ int row[SIDE];
  __shared__ int top[IDS];
  const int n = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
  const int* lab = labels + ((size_t)n * H + y) * W;
  int* d = d2 + ((size_t)n * H + y) * W;
  for (int x = tid; x < W; x += NT) row[x] = d[x];
  for (int i = tid; i < IDS; i += NT) top[i] = 0;
  __syncthreads();
  for (int x = tid; x < W; x += NT) {
    const int id = split_id(lab[x]);
    int best = 0;
    if (id) {
      best = row_distance2(row, W, x, y);
      if (top[id] < best + 2) atomicMax(&top[id], best + 2);
    }
    d[x] = best;
  }
  __syncthreads();
  for (int i = tid; i < IDS; i += NT)
    if (top[i]) atomicMax(m2 + (size_t)n * PAD + i, top[i]);
}

// grid (tiles of an image, images; an image loop when the grid would be too large).  key = the id of a core pixel, 0 elsewhere;
// two touching core pixels are linked when their keys are equal.  area[] is cleared.
__global__ __launch_bounds__(NT) void split_core_tiles_kernel(const int* __restrict__ labels, const int* __restrict__ d2, const int* __restrict__ m2,
                                                              long long num2, long long den2, int N, int H, int W, int tiles_x, int* __restrict__ par,
                                                              int* __restrict__ area) {
  __shared__ int lab[T * T];
  __shared__ int key[T * T];
  const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * T, x0 = tx * T;
  const size_t HW = (size_t)H * W;
  const auto same = [&](int a, int b) { return key[a] == key[b]; };
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const size_t base = (size_t)n * HW;
    for (int l = tid; l < T * T; l += NT) {
      const int y = y0 + l / T, x = x0 + l % T;
      int k = 0;
      if (y < H && x < W) {
        const size_t p = base + (size_t)y * W + x;
        const int id = split_id(labels[p]), dd = d2[p];
        if (id && dd > 0 && den2 * dd > num2 * (m2[(size_t)n * PAD + id] - 2)) k = id;
        area[p] = 0;
      }
      key[l] = k;
    }
    __syncthreads();
    for (int l = tid; l < T * T; l += NT) lab[l] = cc_run_parent<T, NT>(l, key[l] > 0, same);
    __syncthreads();
    for (int l = tid; l < T * T; l += NT) cc_tile_unions<8, T>(lab, l, same);
    __syncthreads();
    for (int l = tid; l < T * T; l += NT) {
      const int y = y0 + l / T, x = x0 + l % T;
      if (y >= H || x >= W) continue;
      par[base + (size_t)y * W + x] = lab[l] >= 0 ? cc_tile_root<T>(lab, l, base, y0, x0, W) : -1;
    }
    __syncthreads();                                                 // lab and key are reused by the next image
  }
}

__global__ __launch_bounds__(NT) void split_join_kernel(const int* __restrict__ labels, int* par, int N, int H, int W) {
  const long long total = (long long)N * H * W, p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  // (a core pixel's parent was written by the launch before and stays >= 0; its label is an id in range)
  cc_join_borders<8, T>(par, p, H, W, [par](long long q) { return par[q] >= 0; }, [labels](long long a, long long b) { return labels[a] == labels[b]; });
}

// grid (chunks, images): every core pixel points at its root, area[root] counts it; a run of equal roots over consecutive lanes is one atomic.
__global__ __launch_bounds__(NT) void split_flatten_kernel(int* par, int* __restrict__ area, int H, int W) {
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    int r = -1;
    if (q < HW && par[base + q] >= 0) r = cc_flatten(par, (long long)(base + q));
    if (__ballot(r >= 0) == 0ull) continue;                       // (wave-uniform)
    const int prev = __shfl_up(r, 1, 64);
    const bool head = lane == 0 || prev != r;
    const int end = run_end(head, lane);
    if (head && r >= 0) atomicAdd(area + r, end - lane);
  }
}

// grid (chunks, images): ncore[id] = the id's cores of at least min_core pixels; dropped = the smaller cores of the image
__global__ __launch_bounds__(NT) void split_cores_kernel(const int* __restrict__ labels, const int* __restrict__ par, const int* __restrict__ area, int H,
                                                         int W, int min_core, int* __restrict__ ncore, int* __restrict__ dropped) {
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  int nd = 0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    if (q >= HW) continue;
    const size_t p = base + q;
    if (par[p] != (int)p) continue;
    if (area[p] >= min_core) atomicAdd(ncore + (size_t)n * PAD + split_id(labels[p]), 1);
    else ++nd;
  }
  nd = wave_sum_int(nd);
  if (lane == 0 && nd) atomicAdd(dropped + n, nd);
}

// one block per image.  An id qualifies with two kept cores; the first max_split of them in id order are the slots.  parts[id] = the
// kept cores of a split id, 1 for any other id with a pixel, 0 for one without; first[id] = the parts of the ids before it.
__global__ __launch_bounds__(NT) void split_ids_kernel(const int* __restrict__ m2, const int* __restrict__ ncore, int max_split, int* __restrict__ parts,
                                                       int* __restrict__ first, int* __restrict__ slot_of, int* __restrict__ slot_id,
                                                       const int* __restrict__ dropped, int* __restrict__ counts) {
  __shared__ int wcount[NT / 64];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int* mm = m2 + (size_t)n * PAD;
  const int* nc = ncore + (size_t)n * PAD;
  int* pt = parts + (size_t)n * PAD;
  int* so = slot_of + (size_t)n * PAD;
  int* sid = slot_id + (size_t)n * SLOTS;
  if (tid < SLOTS) sid[tid] = 0;
  __syncthreads();
  const int qualifying = label_compact<NT>(IDS, wcount, [&](int r) { return r > 0 && nc[r] >= 2; }, [&](int r, int rank) {
    const bool split = rank >= 0 && rank < max_split;
    so[r] = split ? rank : -1;
    if (split) sid[rank] = r;
    pt[r] = (r > 0 && mm[r] > 0) ? (split ? nc[r] : 1) : 0;
  });
  __syncthreads();
  const int total = label_scan<NT>(pt, IDS, first + (size_t)n * PAD, wcount);
  if (tid == 0) {
    const int split = min(qualifying, max_split);
    counts[4 * n] = total; counts[4 * n + 1] = split; counts[4 * n + 2] = dropped[n]; counts[4 * n + 3] = qualifying - split;
  }
}

// grid (chunks, images): chunk[image][slot][chunk] = the kept roots of the slot's id in the chunk
__global__ __launch_bounds__(NT) void split_count_kernel(const int* __restrict__ labels, const int* __restrict__ par, const int* __restrict__ area, int H,
                                                         int W, int min_core, int max_split, const int* __restrict__ slot_of, int* __restrict__ chunk) {
  __shared__ int s[SLOTS];
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  if (tid < SLOTS) s[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    if (q >= HW) continue;
    const size_t p = base + q;
    if (par[p] != (int)p || area[p] < min_core) continue;
    const int slot = slot_of[(size_t)n * PAD + split_id(labels[p])];
    if (slot >= 0) atomicAdd(&s[slot], 1);
  }
  __syncthreads();
  if (tid < max_split) chunk[((size_t)n * max_split + tid) * gridDim.x + blockIdx.x] = s[tid];
}

// grid (max_split, images): a slot's chunk counts become their exclusive prefix
__global__ __launch_bounds__(NT) void split_scan_kernel(int* __restrict__ chunk, int chunks) {
  __shared__ int s[NT];
  block_chunk_prefix<NT>(chunk + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * chunks, chunks, s, [](int) {});
}

// grid (chunks, images): rid[root] of the kept roots of every slot, in the row-major order of the roots; out = first[id] + 1 on
// the pixels of an id that stays whole and 0 on the background (the pixels of a split id are the nearest launch's); the image's
// table rows cleared.
__global__ __launch_bounds__(NT) void split_rank_kernel(const int* __restrict__ labels, const int* __restrict__ par, const int* __restrict__ area, int H,
                                                        int W, int min_core, int max_split, const int* __restrict__ chunk, const int* __restrict__ first,
                                                        const int* __restrict__ slot_of, const int* __restrict__ slot_id, const int* __restrict__ counts,
                                                        int max_instances, int* __restrict__ rid, int* __restrict__ out,
                                                        unsigned long long* __restrict__ table) {
  __shared__ int wcount[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  emit_clear_rows<NT>(table + (size_t)n * max_instances * 8, counts[4 * n], max_instances);
  int slot[PPT], before_id[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    slot[j] = -1; before_id[j] = 0;
    if (q >= HW) continue;
    const size_t p = base + q;
    const int id = split_id(labels[p]);
    const int s = id ? slot_of[(size_t)n * PAD + id] : -1;
    if (s < 0) out[p] = id ? first[(size_t)n * PAD + id] + 1 : 0;
    else if (par[p] == (int)p && area[p] >= min_core) { slot[j] = s; before_id[j] = first[(size_t)n * PAD + id]; }
  }
  for (int s = 0; s < max_split; ++s) {
    if (slot_id[(size_t)n * SLOTS + s] == 0) break;                // (the whole block: the slots fill from 0)
    int running = chunk[((size_t)n * max_split + s) * gridDim.x + blockIdx.x];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      int total;
      const int before = block_rank<NT>(slot[j] == s, wcount, total);
      if (slot[j] == s) rid[base + blockIdx.x * CHUNK + j * NT + tid] = before_id[j] + running + before + 1;
      running += total;
      __syncthreads();
    }
  }
}

// Image blockIdx.y's rows of the table from out, the block's chunk of 1024 pixels of them; Sq from pred, 0 when it is null.  Every
// thread of a grid (chunks, images) calls (split_table_kernel, and split_merge.hip's table launch).
__device__ __forceinline__ void table_rows(EmitSlots& slots, const float* __restrict__ pred, long long stride, const int* __restrict__ out, int H, int W,
                                           int max_instances, unsigned long long* __restrict__ table) {
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  emit_slots_clear(slots);
  __syncthreads();
  unsigned long long* rows = table + (size_t)n * max_instances * 8;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    int k = 0, qv = 0;
    if (q < HW) {
      const int id = out[base + q];
      if (id > 0 && id <= max_instances) {                          // (ids past the table keep their label and have no row)
        k = id;
        if (pred) qv = quantise_u8(pred[(size_t)n * stride + q]);
      }
    }
    emit_record(slots, rows, k, q, W, qv);
  }
  __syncthreads();
  emit_slots_flush(slots, rows);
}

// grid (chunks, images): the table's rows from out
__global__ __launch_bounds__(NT) void split_table_kernel(const float* __restrict__ pred, long long stride, const int* __restrict__ out, int H, int W,
                                                         int max_instances, unsigned long long* __restrict__ table) {
  __shared__ EmitSlots slots;
  table_rows(slots, pred, stride, out, H, W, max_instances, table);
}

unsigned blocks_of(long long count) { return (unsigned)((count + NT - 1) / NT); }

}  // namespace
