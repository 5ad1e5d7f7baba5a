// Reductions over a label map, stated once for rg_features.hip, rg_batch.hip, rg_targets.hip, slic.hip, instances.hip, inst_match.hip and rle.hip
// (DESIGN.md 10k).  The kernels stay in those files with their grids, LDS arrays and side effects; these are the device-inline pieces they share:
//
//   label_slot           a label's slot in a tile's LDS hash table, -1 when the table is full
//   run_end              where the run of equal keys a lane is in ends, over consecutive lanes of a wave
//   block_rank           the kept threads before a thread in one pass of its block, and the pass total
//   block_chunk_prefix   a block's exclusive prefix over an array of counts, in place, with a carry
//   label_compact        ranks of the kept labels among 0 .. n, a block-wide pass at a time with the base carried
//   label_scan           exclusive prefix of n counts, a block-wide pass at a time with the base carried
//   rg_visit_neighbours  a pixel's 12 neighbour offsets: which feed the RAG, the perimeter and the ring sums
//   rg_edge_weight       the weight of a region-graph edge from the two nodes' features
//   rg_emit_row          one wave writes a label's edges (i, j), (j, i) in increasing order of the neighbour
//   rg_store_features    a region's 15 features from its finished statistics
//
// The pieces take functors and template constants, never a flag that says which kernel is calling.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "rg_features.h"      // RGF_NFEAT

// The slot of label k in a tile's table of SLOTS keys (free: -1), or -1 when the table is full and k is not in it.  The table only
// fills, so a label that once got a slot is found there by every later lookup, and one that met a full table never gets one: the
// caller adds straight to memory then, and the same integers reach the same sum.  Any thread calls, between the barrier after the
// caller has set keys[] to -1 and the barrier before it flushes the table; the payload beside keys[] is the caller's.
template <int SLOTS>
__device__ __forceinline__ int label_slot(int* keys, int k) {
  static_assert(SLOTS > 1 && (SLOTS & (SLOTS - 1)) == 0, "the hash keeps the top log2(SLOTS) bits");
  const unsigned h = ((unsigned)k * 0x9E3779B1u) >> (32 - __builtin_ctz(SLOTS));
  int slot = -1;
  for (int t = 0; t < SLOTS; ++t) {
    const int s = (h + t) & (SLOTS - 1);
    const int prev = atomicCAS(&keys[s], -1, k);
    if (prev == -1 || prev == k) { slot = s; break; }
  }
  return slot;
}

// Runs of consecutive lanes with the same key (`head`: the lane starts a run): the lane one past the end of the calling lane's run.
// Every lane of the wave calls.
__device__ __forceinline__ int run_end(bool head, int lane) {
  const unsigned long long hm = __ballot(head);
  const unsigned long long above = lane < 63 ? hm >> (lane + 1) : 0ull;
  return above ? lane + __ffsll((long long)above) : 64;
}

// One pass of a block of NT threads, every thread calls: -> how many threads before this one have `kept` set; total: how many have
// it in all.  wcount is NT / 64 ints of LDS, free again after the caller's next barrier.
template <int NT>
__device__ __forceinline__ int block_rank(bool kept, int* wcount, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(kept);
  if (lane == 0) wcount[wave] = __popcll(mask);
  __syncthreads();
  int before = __popcll(mask & ((1ull << lane) - 1));
  total = 0;
  for (int i = 0; i < NT / 64; ++i) {
    if (i < wave) before += wcount[i];
    total += wcount[i];
  }
  return before;
}

// c[0 .. chunks) becomes its exclusive prefix (Hillis-Steele, NT entries at a time with a carry); every thread of a block of NT
// calls, s is NT ints of LDS.  each(i) runs once for every chunk i, in the thread that loads c[i]: what else the caller sums over
// the chunks rides on the same pass.  -> the total
template <int NT, class Each>
__device__ __forceinline__ int block_chunk_prefix(int* __restrict__ c, int chunks, int* s, Each each) {
  const int tid = threadIdx.x;
  int carry = 0;
  for (int c0 = 0; c0 < chunks; c0 += NT) {
    const int v = c0 + tid < chunks ? c[c0 + tid] : 0;
    if (c0 + tid < chunks) each(c0 + tid);
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
      const int t = tid >= d ? s[tid - d] : 0;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    if (c0 + tid < chunks) c[c0 + tid] = carry + s[tid] - v;
    carry += s[NT - 1];
    __syncthreads();
  }
  return carry;
}

// Labels 0 .. n in passes of NT with the base carried from pass to pass: each(r, rank) runs once for every r < n, rank = the kept
// labels in front of r when keep(r), else -1.  Every thread of ONE block of NT calls (rgf_finalize_kernel, rgb_rank_kernel); wcount
// as for block_rank.  each runs between block_rank's barrier and the barrier that ends the pass, which frees wcount.  -> the kept labels
template <int NT, class Keep, class Each>
__device__ __forceinline__ int label_compact(int n, int* wcount, Keep keep, Each each) {
  int base = 0;
  for (int r0 = 0; r0 < n; r0 += NT) {
    const int r = r0 + threadIdx.x;
    const bool kept = r < n && keep(r);
    int total;
    const int before = block_rank<NT>(kept, wcount, total);
    if (r < n) each(r, kept ? base + before : -1);
    base += total;
    __syncthreads();
  }
  return base;
}

// out[r] = in[0] + .. + in[r - 1] for r < n, in passes of NT with the base carried.  Every thread of ONE block of NT calls
// (rgf_scan_kernel, rgb_scan_kernel, rle_scan_kernel); wsum is NT / 64 ints of LDS, written before the pass's first barrier and free after its
// second.  -> the total, which the caller stores where it wants it
template <int NT>
__device__ __forceinline__ int label_scan(const int* __restrict__ in, int n, int* __restrict__ out, int* wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;
  for (int r0 = 0; r0 < n; r0 += NT) {
    const int r = r0 + threadIdx.x;
    const int v = r < n ? in[r] : 0;
    const int inc = wave_scan_int(v);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = base;
    for (int i = 0; i < NT / 64; ++i) {
      if (i < wave) off += wsum[i];
      base += wsum[i];
    }
    if (r < n) out[r] = off + inc - v;
    __syncthreads();
  }
  return base;
}

// The neighbours of a pixel with label r that region-graph construction looks at: the offsets within L1 distance 2, in rings (the
// 4-neighbours first, then the other 8); offsets 0-3 and 8-11 are the 8-neighbourhood.  Called per pixel by rgf_accumulate_kernel
// and rgb_accumulate_kernel; no LDS, no barrier.  The offsets are compile-time constants of the unrolled loop.
//   label_at(dy, dx)   the neighbour's label, negative where there is none (outside the image, a label out of range)
//   on_rag(l)          every foreign label of the 8-neighbourhood, on every occurrence: (r, l) is a RAG edge
//   on_first(l, four)  once per distinct foreign label: the pixel is in l's ring; `four`: l was first seen among the 4-neighbours,
//                      so the pixel is on l's dilation and counts for l's perimeter
template <class LabelAt, class OnRag, class OnFirst>
__device__ __forceinline__ void rg_visit_neighbours(int r, LabelAt label_at, OnRag on_rag, OnFirst on_first) {
  const int dy[12] = {-1, 1, 0, 0, -2, 2, 0, 0, -1, -1, 1, 1};
  const int dx[12] = {0, 0, -1, 1, 0, 0, -2, 2, -1, 1, -1, 1};
  int seen[12]; int nseen = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const int l = label_at(dy[k], dx[k]);
    if (l == r || l < 0) continue;
    if (k < 4 || k >= 8) on_rag(l);
    bool dup = false;
    for (int s = 0; s < nseen; ++s) dup |= (seen[s] == l);
    if (dup) continue;
    seen[nseen++] = l;
    on_first(l, k < 4);
  }
}

// the reference's edge weight [:226-234] from the two nodes' feature rows, in fp32
__device__ __forceinline__ float rg_edge_weight(const float* __restrict__ xi, const float* __restrict__ xj) {
  const float d0 = xi[0] - xj[0], d1 = xi[1] - xj[1], d2 = xi[2] - xj[2];
  const float color = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  return expf(-color / 0.15f) * expf(-fabsf(xi[6] - xj[6]) / 0.08f) * expf(-fabsf(xi[12] - xj[12]) / 0.1f);
}

// The edges of label a, node i, to its neighbours b > a in increasing b: undirected edge number pos onwards, each as (i, j) and
// (j, i) with one weight; nothing is written at or past edge_capacity.  One WAVE calls, all 64 lanes (rgf_emit_kernel,
// rgb_emit_kernel); no LDS.  on(b), for a < b < n_labels: b is adjacent to a and kept; node(b): its row of x.
template <class On, class Node>
__device__ __forceinline__ void rg_emit_row(int a, int n_labels, long long pos, int i, const float* __restrict__ x, On on, Node node,
                                            long long* __restrict__ edge_index, float* __restrict__ edge_attr, int edge_capacity) {
  const int lane = threadIdx.x & 63;
  const float* xi = x + (size_t)i * RGF_NFEAT;
  for (int b0 = a + 1; b0 < n_labels; b0 += 64) {
    const int b = b0 + lane;
    const bool hit = b < n_labels && on(b);
    const unsigned long long bal = __ballot(hit);
    if (hit) {
      const int j = node(b);
      const long long e = 2ll * (pos + __popcll(bal & ((1ull << lane) - 1ull)));
      const float wgt = rg_edge_weight(xi, x + (size_t)j * RGF_NFEAT);
      if (e + 1 < edge_capacity) {
        edge_index[e] = i; edge_index[e + 1] = j;
        edge_index[(size_t)edge_capacity + e] = j; edge_index[(size_t)edge_capacity + e + 1] = i;
        edge_attr[e] = wgt; edge_attr[e + 1] = wgt;
      }
    }
    pos += __popcll(bal);
  }
}

// A kept region's feature row [:201-212] from its FINISHED statistics: colour and luma means, their variances (clamped at 0 by the
// caller, whose arithmetic they are), mean x and y, pixel count, perimeter, contrast against the ring, share of edge pixels.
struct RgStats {
  double mr, mg, mb, ml, vr, vg, vb, vl, mx, my, n, perim, contrast, edge;
};
__device__ __forceinline__ void rg_store_features(float* __restrict__ o, const RgStats& s) {
  o[0] = (float)s.mr; o[1] = (float)s.mg; o[2] = (float)s.mb;
  o[3] = (float)sqrt(s.vr); o[4] = (float)sqrt(s.vg); o[5] = (float)sqrt(s.vb);
  o[6] = (float)s.ml; o[7] = (float)sqrt(s.vl);
  o[8] = (float)(s.mx / 256.0); o[9] = (float)(s.my / 256.0);
  o[10] = (float)(s.n / 65536.0);
  o[11] = (float)(s.perim * s.perim / (4.0 * 3.14159265358979323846 * s.n + 1e-10));
  o[12] = (float)s.contrast; o[13] = (float)s.edge; o[14] = (float)s.vl;
}
