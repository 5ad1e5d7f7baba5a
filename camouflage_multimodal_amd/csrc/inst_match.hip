// Instance matching (include/camo_inst_match.h): the pixels of every (predicted id, ground-truth id) pair of two label
// maps, and the greedy matches of predictions to ground truth in score order at each IoU threshold.  8 B/pixel in, one pixel-rate
// pass; the rest works on the small tables.  Every grid covers the whole batch.
//
//   clear    inter and counts to zero
//   overlap  per chunk of 1024 pixels: a run of equal (p, g) over consecutive lanes is one record; records meet in a block's LDS
//            slots (label_inl.h's label_slot; memory when the table is full), the block adds its slots to inter once
//   areas    row sums (one wave per predicted id) and column sums (one thread per ground-truth id) of inter, and every predicted
//            id's rank in score order (one thread per id)
//   match    one block per (threshold, image): predicted ids in rank order, each takes the unmatched ground-truth id of highest IoU
//            at or above the threshold; up to 16 more blocks per image write every prediction's best ground truth and the counts
//
// The match of include/camo_boundary.h under min(mask IoU, boundary IoU) is the same code: clear, overlap and areas
// once more for the table of the two boundary maps, and the match kernel's other instantiation.
// Integer arithmetic only, IoUs compared by cross-multiplication; 32-bit integer atomic adds only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "common.h"
#include "inst_match.h"
#include "instances.h"
#include "label_inl.h"
#include "../../include/camo_inst_match.h"
#include "../../include/camo_boundary.h"

namespace {

constexpr int NT = INST_NT, CHUNK = INST_CHUNK, PPT = INST_CHUNK / INST_NT, WAVES = NT / 64;
constexpr int SLOTS = 32;                  // pairs a block of the overlap launch sums in LDS
constexpr int MAX_IDS = CAMO_IM_MAX_IDS;
static_assert(CHUNK % NT == 0 && NT % 64 == 0, "whole waves, whole passes");
static_assert(IM_MAX_THRESHOLDS == CAMO_IM_MAX_THRESHOLDS, "the kernel argument holds every threshold");

__global__ __launch_bounds__(NT) void im_clear_kernel(int* __restrict__ inter, long long cells, int* __restrict__ counts, int ncounts) {
  const long long step = (long long)gridDim.x * NT;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < cells; i += step) inter[i] = 0;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < ncounts; i += NT) counts[i] = 0;
}

// grid (chunks, images).  key = p (G + 1) + g of a pixel with both labels in range, -1 otherwise (counted in counts[0], counts[1]).
__global__ __launch_bounds__(NT) void im_overlap_kernel(const int* __restrict__ pl, const int* __restrict__ gl, int HW, int P, int G,
                                                        int* __restrict__ inter, int* __restrict__ counts) {
  __shared__ int slot_key[SLOTS];                                  // -1: free
  __shared__ int slot_cnt[SLOTS];
  __shared__ int oob[2];
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y;
  const size_t base = (size_t)n * HW;
  if (tid < SLOTS) { slot_key[tid] = -1; slot_cnt[tid] = 0; }
  if (tid < 2) oob[tid] = 0;
  __syncthreads();
  int* cells = inter + (size_t)n * (P + 1) * (G + 1);
  int np = 0, ng = 0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    int key = -1;
    if (q < HW) {
      const int p = pl[base + q], g = gl[base + q];
      const bool pin = (unsigned)p <= (unsigned)P, gin = (unsigned)g <= (unsigned)G;      // (a negative label is out of range)
      np += !pin;
      ng += !gin;
      if (pin && gin) key = p * (G + 1) + g;
    }
    if (__ballot(key >= 0) == 0ull) continue;                      // (wave-uniform)
    const int prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const int len = run_end(head, lane) - lane;
    if (head && key >= 0) {
      const int s = label_slot<SLOTS>(slot_key, key);
      if (s >= 0) atomicAdd(&slot_cnt[s], len);
      else atomicAdd(cells + key, len);
    }
  }
  np = wave_sum_int(np);
  ng = wave_sum_int(ng);
  if (lane == 0) {
    if (np) atomicAdd(&oob[0], np);
    if (ng) atomicAdd(&oob[1], ng);
  }
  __syncthreads();
  if (tid < SLOTS && slot_key[tid] >= 0) atomicAdd(cells + slot_key[tid], slot_cnt[tid]);
  if (tid < 2 && oob[tid]) atomicAdd(counts + CAMO_IM_COUNTS * n + tid, oob[tid]);
}

// The score Sq / area of a row (area, ..., Sq) of camo_instances' table; 0 / 1 when it is not a row.
__device__ __forceinline__ void im_score(long long a, long long s, long long& sq, long long& area) {
  const bool row = a > 0 && a <= CAMO_RGD_MAX_IMAGE_PIXELS && s >= 0 && s <= 255 * a;
  sq = row ? s : 0;
  area = row ? a : 1;
}

// grid (row blocks + column blocks + rank blocks, images).  Row blocks: a wave sums inter's row p.  Column blocks: a thread sums
// column g (consecutive threads, consecutive addresses).  Rank blocks: a thread counts the ids that come before id p.  An id's row of
// pred_rows has row_fields ints (the area goes to the first, the rank to the second), its entry of gt_area gt_fields.
__global__ __launch_bounds__(NT) void im_areas_kernel(const int* __restrict__ inter, int P, int G, const long long* __restrict__ table, int nrows,
                                                      int row_blocks, int col_blocks, int* __restrict__ area_p, int* __restrict__ area_g,
                                                      int* __restrict__ rank, int* __restrict__ pred_rows, int row_fields, int* __restrict__ gt_area,
                                                      int gt_fields) {
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y;
  const int* cells = inter + (size_t)n * (P + 1) * (G + 1);
  int b = blockIdx.x;
  if (b < row_blocks) {
    const int p = b * WAVES + (tid >> 6);
    if (p > P) return;                                             // (the whole wave)
    int s = 0;
    for (int g = lane; g <= G; g += 64) s += cells[(size_t)p * (G + 1) + g];
    s = wave_sum_int(s);
    if (lane == 0) {
      area_p[(size_t)n * (P + 1) + p] = s;
      if (p) pred_rows[((size_t)n * P + p - 1) * row_fields] = s;
    }
    return;
  }
  b -= row_blocks;
  if (b < col_blocks) {
    const int g = b * NT + tid;
    if (g > G) return;
    int s = 0;
#pragma unroll 8                                                   // (independent loads: eight in flight)
    for (int p = 0; p <= P; ++p) s += cells[(size_t)p * (G + 1) + g];
    area_g[(size_t)n * (G + 1) + g] = s;
    if (g) gt_area[((size_t)n * G + g - 1) * gt_fields] = s;
    return;
  }
  b -= col_blocks;
  const int p = b * NT + tid + 1;
  if (p > P) return;
  int before = p - 1;                                              // no table: the order is by id
  if (table) {
    const long long* rows = table + (size_t)n * nrows * CAMO_INST_FIELDS;
    const int have = min(P, nrows);                                // ids past the table's rows score 0 / 1
    long long sp = 0, ap = 1;
    if (p <= have) im_score(rows[(size_t)(p - 1) * CAMO_INST_FIELDS], rows[(size_t)(p - 1) * CAMO_INST_FIELDS + 7], sp, ap);
    before = 0;
#pragma unroll 8                                                   // (the rows are the same for every lane: eight pairs of loads in flight)
    for (int q = 1; q <= have; ++q) {
      long long sq, aq;
      im_score(rows[(size_t)(q - 1) * CAMO_INST_FIELDS], rows[(size_t)(q - 1) * CAMO_INST_FIELDS + 7], sq, aq);
      const long long l = sq * ap, r = sp * aq;                    // score q against score p: both below 2^60
      before += l > r || (l == r && q < p);
    }
    if (sp == 0) before += max(0, p - 1 - have);                   // the ids have + 1 .. p - 1 tie with a score of 0 and come first
  }
  rank[(size_t)n * P + p - 1] = before;
  pred_rows[((size_t)n * P + p - 1) * row_fields + 1] = before;
}

// The boundary table of the combined match (BD): inter_bd and its row and column sums.  Nothing for the mask-only match.
template <bool BD> struct ImBoundary {};
template <> struct ImBoundary<true> { const int *inter, *area_p, *area_g; };

// Ground-truth id g as a candidate of a predicted id, from its intersection i and union u in the mask table.  BD: under the smaller
// of that fraction and the boundary table's -- brow the table's row of the predicted id, b its boundary area, bg the ground truth's.
template <bool BD>
__device__ __forceinline__ ImCand im_cand(int i, int u, int g, const int* __restrict__ brow, int b, const int* bg) {
  if constexpr (BD) {
    const int ib = brow[g];
    return bd_cand(i, u, ib, b + bg[g] - ib, g);
  } else {
    return ImCand{i, u, g};
  }
}

// The blocks past the thresholds' (block e of E): every prediction's ground-truth id of highest IoU, matched or not, one wave per
// predicted id, with the intersection (BD: the two intersections) to fields 2, 3 (and 5) of its row of `rows`; block 0 also counts the
// ids in use, from the mask table's areas.  ap, ag, bp, bg: the areas in LDS; used: two zeroed ints of LDS.
template <bool BD>
__device__ __forceinline__ void im_best_rows(const int* __restrict__ cells, const int* __restrict__ bcells, int P, int G, const int* ap,
                                             const int* ag, const int* bp, const int* bg, int* used, int e, int E, int* __restrict__ rows,
                                             int* __restrict__ counts) {
  constexpr int FIELDS = BD ? CAMO_BD_ROW_FIELDS : 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int p = e * WAVES + wave + 1; p <= P; p += E * WAVES) {
    const int a = ap[p], b = BD ? bp[p] : 0;
    const int* row = cells + (size_t)p * (G + 1);
    const int* brow = BD ? bcells + (size_t)p * (G + 1) : nullptr;
    ImCand best{0, 1, 0};
    if (a)
      for (int g = lane + 1; g <= G; g += 64) {
        const int i = row[g];
        if (i <= 0) continue;
        const ImCand c = im_cand<BD>(i, a + ag[g] - i, g, brow, b, bg);
        if (im_before(c, best)) best = c;
      }
    best = im_wave_best(best);
    if (lane == 0) {
      rows[(size_t)(p - 1) * FIELDS + 2] = best.g;
      if constexpr (BD) {                                          // (best.i may be either table's)
        rows[(size_t)(p - 1) * FIELDS + 3] = best.g ? row[best.g] : 0;
        rows[(size_t)(p - 1) * FIELDS + 5] = best.g ? brow[best.g] : 0;
      } else {
        rows[(size_t)(p - 1) * FIELDS + 3] = best.i;
      }
    }
  }
  if (e) return;
  int np = 0, ng = 0;
  for (int p = tid + 1; p <= P; p += NT) np += ap[p] > 0;
  for (int g = tid + 1; g <= G; g += NT) ng += ag[g] > 0;
  np = wave_sum_int(np);
  ng = wave_sum_int(ng);
  if (lane == 0) { atomicAdd(&used[0], np); atomicAdd(&used[1], ng); }
  __syncthreads();
  if (tid < 2) counts[2 + tid] = used[tid];
}

// grid (thresholds + row blocks, images).  Thread t owns ground-truth ids t + 1, t + 1 + NT, ...: it alone reads and writes their taken[] flag.
// BD: the match under min(mask IoU, boundary IoU) -- the boundary table's areas beside the mask table's in LDS, a second row read per
// candidate; pred_rows has CAMO_BD_ROW_FIELDS ints a row, not 4.
template <bool BD>
__global__ __launch_bounds__(NT) void im_match_kernel(const int* __restrict__ inter, int P, int G, ImThresholds thr, int T, const int* __restrict__ area_p,
                                                      const int* __restrict__ area_g, const int* __restrict__ rank, int* __restrict__ match,
                                                      int* __restrict__ gt_match, int* __restrict__ pred_rows, int* __restrict__ counts,
                                                      ImBoundary<BD> bd) {
  __shared__ int ap[MAX_IDS + 1], ag[MAX_IDS + 1], taken[MAX_IDS + 1];
  __shared__ int bp[BD ? MAX_IDS + 1 : 1], bg[BD ? MAX_IDS + 1 : 1];      // (not used, and no LDS, without BD)
  __shared__ int order[MAX_IDS];                                   // order[r] = the predicted id of rank r
  __shared__ ImCand wbest[2][WAVES];
  __shared__ int used[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = blockIdx.x, n = blockIdx.y;
  const size_t table = (size_t)n * (P + 1) * (G + 1);
  const int* cells = inter + table;
  const int* bcells = nullptr;
  if constexpr (BD) bcells = bd.inter + table;
  for (int p = tid; p <= P; p += NT) {
    ap[p] = area_p[(size_t)n * (P + 1) + p];
    if constexpr (BD) bp[p] = bd.area_p[(size_t)n * (P + 1) + p];
  }
  for (int g = tid; g <= G; g += NT) {
    ag[g] = area_g[(size_t)n * (G + 1) + g];
    if constexpr (BD) bg[g] = bd.area_g[(size_t)n * (G + 1) + g];
    taken[g] = 0;
  }
  if (k < T)
    for (int p = tid; p < P; p += NT) order[rank[(size_t)n * P + p]] = p + 1;    // (rank is a permutation of 0 .. P - 1)
  if (tid < 2) used[tid] = 0;
  __syncthreads();
  if (k >= T) {                                                    // (the whole block)
    im_best_rows<BD>(cells, bcells, P, G, ap, ag, bp, bg, used, k - T, gridDim.x - T, pred_rows + (size_t)n * P * (BD ? CAMO_BD_ROW_FIELDS : 4),
                     counts + CAMO_IM_COUNTS * n);
    return;
  }

  const long long num = thr.num[k], den = thr.den;
  int* mrow = match + ((size_t)n * T + k) * P;
  int buf = 0;
  for (int r = 0; r < P; ++r) {
    const int p = order[r], a = ap[p], b = BD ? bp[p] : 0;
    if (a == 0) {                                                  // (the whole block: no barrier is skipped by a part of it)
      if (tid == 0) mrow[p - 1] = 0;
      continue;
    }
    const int* row = cells + (size_t)p * (G + 1);
    const int* brow = BD ? bcells + (size_t)p * (G + 1) : nullptr;
    ImCand best{0, 1, 0};
    for (int g = tid + 1; g <= G; g += NT) {
      const int ga = ag[g];
      if (ga == 0 || taken[g]) continue;
      const int i = row[g];
      if (i <= 0) continue;
      const ImCand c = im_cand<BD>(i, a + ga - i, g, brow, b, bg);
      if (den * c.i < num * c.u) continue;
      if (im_before(c, best)) best = c;
    }
    best = im_wave_best(best);
    if (lane == 0) wbest[buf][wave] = best;
    __syncthreads();
    best = wbest[buf][0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      if (im_before(wbest[buf][w], best)) best = wbest[buf][w];
    if (best.g && ((best.g - 1) & (NT - 1)) == tid) taken[best.g] = p;      // (the owner)
    if (tid == 0) mrow[p - 1] = best.g;
    buf ^= 1;      // the next round writes the other half: a wave still reading this one is at most one barrier behind
  }
  for (int g = tid + 1; g <= G; g += NT) gt_match[((size_t)n * T + k) * G + g - 1] = taken[g];
}

// the last launch of either call
template <bool BD>
int launch_im_match(const int* inter, int N, int P, int G, const ImThresholds& thr, int T, const ImWs& ws, int* match, int* gt_match, int* pred_rows,
                    int* counts, ImBoundary<BD> bd, hipStream_t stream) {
  const int best_blocks = std::min((P + WAVES - 1) / WAVES, 16);
  hipLaunchKernelGGL(im_match_kernel<BD>, dim3(T + best_blocks, N), dim3(NT), 0, stream, inter, P, G, thr, T, ws.area_p, ws.area_g, ws.rank, match,
                     gt_match, pred_rows, counts, bd);
  return (int)hipGetLastError();
}

}  // namespace

ImWs im_carve(int N, int P, int G, bool boundary, void* base) {
  ImWs w{};
  camo_abi::Carver c(base);
  w.area_p = c.take<int>((size_t)N * (P + 1));
  w.area_g = c.take<int>((size_t)N * (G + 1));
  w.rank = c.take<int>((size_t)N * P);
  if (boundary) {
    w.bd_area_p = c.take<int>((size_t)N * (P + 1));
    w.bd_area_g = c.take<int>((size_t)N * (G + 1));
    w.bd_counts = c.take<int>((size_t)N * CAMO_IM_COUNTS);
  }
  w.bytes = c.bytes();
  return w;
}

int launch_im_table(const int* pred_labels, const int* gt_labels, int N, int H, int W, int P, int G, const long long* pred_table,
                    int pred_table_rows, bool with_rank, int* area_p, int* area_g, int* rank, int* inter, int* pred_rows, int row_fields,
                    int* gt_area, int gt_fields, int* counts, hipStream_t stream) {
  const int HW = H * W, chunks = (HW + CHUNK - 1) / CHUNK;
  const long long cells = (long long)N * (P + 1) * (G + 1);
  const unsigned clear_blocks = (unsigned)std::min<long long>((cells + NT - 1) / NT, 4096);
  hipLaunchKernelGGL(im_clear_kernel, dim3(clear_blocks), dim3(NT), 0, stream, inter, cells, counts, CAMO_IM_COUNTS * N);
  hipLaunchKernelGGL(im_overlap_kernel, dim3(chunks, N), dim3(NT), 0, stream, pred_labels, gt_labels, HW, P, G, inter, counts);
  const int row_blocks = (P + 1 + WAVES - 1) / WAVES, col_blocks = (G + 1 + NT - 1) / NT, rank_blocks = with_rank ? (P + NT - 1) / NT : 0;
  hipLaunchKernelGGL(im_areas_kernel, dim3(row_blocks + col_blocks + rank_blocks, N), dim3(NT), 0, stream, inter, P, G, pred_table,
                     pred_table_rows, row_blocks, col_blocks, area_p, area_g, rank, pred_rows, row_fields, gt_area, gt_fields);
  return (int)hipGetLastError();
}

int launch_inst_match(const int* pred_labels, const int* gt_labels, int N, int H, int W, int P, int G, const long long* pred_table,
                      int pred_table_rows, const ImThresholds& thr, int T, const ImWs& ws, int* inter, int* pred_rows, int* gt_area,
                      int* match, int* gt_match, int* counts, hipStream_t stream) {
  if (int e = launch_im_table(pred_labels, gt_labels, N, H, W, P, G, pred_table, pred_table_rows, true, ws.area_p, ws.area_g, ws.rank, inter,
                              pred_rows, 4, gt_area, 1, counts, stream))
    return e;
  return launch_im_match<false>(inter, N, P, G, thr, T, ws, match, gt_match, pred_rows, counts, {}, stream);
}

int launch_boundary_match(const int* pred_labels, const int* gt_labels, const int* pred_bd, const int* gt_bd, int N, int H, int W, int P, int G,
                          const long long* pred_table, int pred_table_rows, const ImThresholds& thr, int T, const ImWs& ws, int* inter,
                          int* inter_bd, int* pred_rows, int* gt_area, int* match, int* gt_match, int* counts, hipStream_t stream) {
  // the mask table: areas to fields 0 of pred_rows and gt_area, ranks to field 1; the boundary table: areas to fields 4 and 1
  if (int e = launch_im_table(pred_labels, gt_labels, N, H, W, P, G, pred_table, pred_table_rows, true, ws.area_p, ws.area_g, ws.rank, inter, pred_rows,
                              CAMO_BD_ROW_FIELDS, gt_area, CAMO_BD_GT_FIELDS, counts, stream))
    return e;
  if (int e = launch_im_table(pred_bd, gt_bd, N, H, W, P, G, nullptr, 0, false, ws.bd_area_p, ws.bd_area_g, nullptr, inter_bd, pred_rows + 4,
                              CAMO_BD_ROW_FIELDS, gt_area + 1, CAMO_BD_GT_FIELDS, ws.bd_counts, stream))
    return e;
  return launch_im_match<true>(inter, N, P, G, thr, T, ws, match, gt_match, pred_rows, counts, {inter_bd, ws.bd_area_p, ws.bd_area_g}, stream);
}
