// The instance table of a label map (include/camo_instances.h item 8), stated once for instances.hip and split.hip.
// The kernels stay in those files with their grids and side effects; these are the device-inline pieces they share:
//
//   emit_clear_rows    an image's table rows cleared, the box minima of the rows in use to the largest value
//   emit_slots_clear   a block's LDS slots made free, before a barrier
//   emit_record        one pass of a wave over 64 consecutive pixels: a run of equal ids over consecutive lanes inside one image row is
//                      one record (len, x, y, sum of q) whose sums have closed forms.  A record goes to the id's slot of a small LDS
//                      table (open addressing from id mod EMIT_SLOTS; to the table in memory when every slot is another id's)
//   emit_slots_flush   after a barrier: the block adds its slots to the table in memory once -- a block of one large object costs
//                      eight atomics, whatever else crosses its rows
//
// 64-bit integer atomics only: the table is a function of the label map and the prediction, whatever the order.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "label_inl.h"

constexpr int EMIT_SLOTS = 16;
constexpr unsigned long long EMIT_BOX_MIN_INIT = 0x7fffffffffffffffull;

struct EmitSlots {
  int id[EMIT_SLOTS];                                              // 0: free
  unsigned long long row[EMIT_SLOTS][8];
};

// rows: the image's max_instances x 8 cells; K: the ids it holds.  Every thread of a grid row of gridDim.x blocks of NT calls.
template <int NT>
__device__ __forceinline__ void emit_clear_rows(unsigned long long* __restrict__ rows, long long K, int max_instances) {
  const long long cells = (long long)max_instances * 8;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < cells; i += (long long)gridDim.x * NT) {
    const int f = (int)(i & 7);
    rows[i] = ((i >> 3) < K && (f == 1 || f == 2)) ? EMIT_BOX_MIN_INIT : 0ull;
  }
}

// every thread of a block of at least EMIT_SLOTS * 8 threads calls, before a barrier
__device__ __forceinline__ void emit_slots_clear(EmitSlots& s) {
  const int tid = threadIdx.x;
  if (tid < EMIT_SLOTS) s.id[tid] = 0;
  if (tid < EMIT_SLOTS * 8) s.row[tid >> 3][tid & 7] = ((tid & 7) == 1 || (tid & 7) == 2) ? EMIT_BOX_MIN_INIT : 0ull;
}

// Every lane of a wave calls with pixel q of the image (consecutive over the lanes): k its id when it has a row of the table, else 0
// (k > 0 only inside the image); qv: its quantised prediction (read where k > 0).
__device__ __forceinline__ void emit_record(EmitSlots& s, unsigned long long* __restrict__ rows, int k, int q, int W, int qv) {
  if (__ballot(k > 0) == 0ull) return;                            // (wave-uniform)
  const int lane = threadIdx.x & 63;
  const int y = q / W, x = q - y * W;
  qv = k > 0 ? qv : 0;
  const int prev = __shfl_up(k, 1, 64);
  const bool head = lane == 0 || prev != k || x == 0;
  const int end = run_end(head, lane), len = end - lane;
  const int pre = wave_scan_int(qv);                               // inclusive prefix of q over the wave (at most 64 * 255)
  const int sq = __shfl(pre, end - 1, 64) - (pre - qv);
  if (head && k > 0) {                                             // (no branch around the shuffles above: every lane takes them)
    const unsigned long long sx = (unsigned long long)len * x + (unsigned long long)len * (len - 1) / 2, sy = (unsigned long long)len * y;
    unsigned long long* row = rows + (size_t)(k - 1) * 8;          // the table in memory, unless a slot takes the record
    int t = k & (EMIT_SLOTS - 1);
    for (int probe = 0; probe < EMIT_SLOTS; ++probe, t = (t + 1) & (EMIT_SLOTS - 1)) {
      const int old = atomicCAS(&s.id[t], 0, k);
      if (old == 0 || old == k) { row = s.row[t]; break; }
    }
    atomicAdd(row + 0, (unsigned long long)len);
    atomicMin(row + 1, (unsigned long long)x);
    atomicMin(row + 2, (unsigned long long)y);
    atomicMax(row + 3, (unsigned long long)(x + len - 1));
    atomicMax(row + 4, (unsigned long long)y);
    atomicAdd(row + 5, sx);
    atomicAdd(row + 6, sy);
    atomicAdd(row + 7, (unsigned long long)sq);
  }
}

// every thread of the block calls, after the barrier that follows its last emit_record
__device__ __forceinline__ void emit_slots_flush(EmitSlots& s, unsigned long long* __restrict__ rows) {
  const int tid = threadIdx.x;
  if (tid >= EMIT_SLOTS * 8) return;
  const int k = s.id[tid >> 3], f = tid & 7;
  if (k == 0) return;
  const unsigned long long v = s.row[tid >> 3][f];
  unsigned long long* cell = rows + (size_t)(k - 1) * 8 + f;
  if (f == 1 || f == 2) atomicMin(cell, v);
  else if (f == 3 || f == 4) atomicMax(cell, v);
  else atomicAdd(cell, v);
}
