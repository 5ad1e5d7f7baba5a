// Boundary IoU (include/camo_boundary.h): the boundary region of every instance of a label map -- the instance minus
// its erosion by a (2d + 1)^2 square, the image border counting as outside -- and the greedy match of inst_match.hip under
// min(mask IoU, boundary IoU).  The erosion is separable and runs on runs of equal labels, so its cost does not follow d:
//
//   row     one wave per image row, 64 pixels a step: the run of equal labels a pixel is in, from two ballots, carried from step to step
//           along the row and never past its end; rowok = the run reaches d to the left and d to the right; one byte per pixel
//   column  one thread per column of a strip of BD_STRIP rows: over the key (the label where rowok, else none) the run of equal keys
//           must reach d up and d down; one sweep up the strip leaves a bit per row, one sweep down writes out
//   match   im_match_kernel with the boundary table's areas beside the mask table's in LDS and a second row read per candidate
//
// The two tables of the match come from inst_match.hip's clear, overlap and areas launches (launch_im_table), once per pair of maps.
// Integer arithmetic only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "boundary.h"
#include "common.h"
#include "label_inl.h"
#include "../../include/camo_boundary.h"

namespace {

constexpr int NT = BD_NT, WAVES = NT / 64, STRIP = BD_STRIP;
constexpr int MAX_IDS = CAMO_IM_MAX_IDS;
static_assert(STRIP == 64 && STRIP == CAMO_BD_STRIP, "one bit of a 64-bit mask per row of a strip; include/camo_boundary.h states it");
static_assert(NT % 64 == 0, "whole waves");

// grid (ceil(H / WAVES), images): a wave takes one row.  A run [s, e) of equal labels gives rowok(x) = x - s >= d && e - 1 - x >= d.
// A run that is still open at the end of a step is not written then: `open`, `cs` (its start) and `cl` (its label) carry it, and the
// step that sees it end writes its pixels of the earlier steps.  Every byte of the row is written exactly once.
__global__ __launch_bounds__(NT) void bd_row_kernel(const int* __restrict__ labels, int H, int W, int d, unsigned char* __restrict__ rowok) {
  const int lane = threadIdx.x & 63, y = blockIdx.x * WAVES + (threadIdx.x >> 6), n = blockIdx.y;
  if (y >= H) return;                                              // (the whole wave)
  const size_t base = ((size_t)n * H + y) * W;
  const int* row = labels + base;
  unsigned char* ok = rowok + base;
  bool open = false;
  int cs = 0, cl = 0;
  int next = lane < W ? row[lane] : 0;
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + lane;
    const bool in = x < W, last = x0 + 64 >= W;
    const int L = next;
    if (!last) next = x + 64 < W ? row[x + 64] : 0;                // (the next step's labels are on their way while this one works)
    const int prev = __shfl_up(L, 1, 64);
    const bool head = lane == 0 || prev != L || !in;               // a lane past the row is a run of its own: the row's last run ends at W
    const int le = run_end(head, lane);
    const int ls = 63 - __clzll((long long)(__ballot(head) & (~0ull >> (63 - lane))));      // the mirrored ballot: the last head at or below the lane
    const int L0 = __builtin_amdgcn_readfirstlane(L), le0 = __builtin_amdgcn_readfirstlane(le);
    const bool cont = open && L0 == cl;
    if (open && (!cont || le0 < 64 || last)) {                     // (wave-uniform) the carried run ends here: at x0, or inside this step
      const int e = cont ? x0 + le0 : x0;
      for (int xx = cs + lane; xx < x0; xx += 64) ok[xx] = (xx - cs >= d && e - 1 - xx >= d) ? 1 : 0;
    }
    const int s = (ls == 0 && cont) ? cs : x0 + ls, e = x0 + le;
    if (in && (le < 64 || last)) ok[x] = (x - s >= d && e - 1 - x >= d) ? 1 : 0;
    open = !last;
    cs = __builtin_amdgcn_readlane(s, 63);
    cl = __builtin_amdgcn_readlane(L, 63);
  }
}

// grid (ceil(W / NT), ceil(H / STRIP), images): thread = column x of a strip of rows [y0, y1).  key(y) = the label where it is positive
// and rowok, else 0.  A pixel is interior when its key is not 0 and the vertical run of equal keys reaches d up and d down.  The runs
// leave the strip: the rows below y1 - 1 with its key are counted first (at most d of them, none when the key is 0), then a sweep up
// the strip sets bit y - y0 where the run reaches d down; the same above y0, and a sweep down writes out.  rowok null: 2d + 1 exceeds
// a side, no pixel is interior and the row pass did not run.
__global__ __launch_bounds__(NT) void bd_col_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ rowok, int H, int W, int d,
                                                    int* __restrict__ out) {
  const int x = blockIdx.x * NT + threadIdx.x, y0 = blockIdx.y * STRIP, y1 = min(y0 + STRIP, H), n = blockIdx.z;
  if (x >= W) return;
  const size_t img = (size_t)n * H * W + x;
  if (!rowok) {                                                    // (the whole grid)
    for (int y = y0; y < y1; ++y) out[img + (size_t)y * W] = max(labels[img + (size_t)y * W], 0);
    return;
  }
  auto key = [&](int y) {                                          // (two loads and no branch: the sweeps below keep eight rows in flight)
    const size_t q = img + (size_t)y * W;
    const int L = labels[q];
    return ((rowok[q] != 0) & (L > 0)) ? L : 0;
  };
  unsigned long long down = 0ull;
  {
    const int kb = key(y1 - 1);
    int dn = 0;
    if (kb)
      for (int y = y1; y < H && dn < d && key(y) == kb; ++y) ++dn;
    int pk = kb, cnt = dn - 1;                                       // the first step below finds its own key and makes cnt = dn
#pragma unroll 8                                                   // (the loads do not depend on the counting: eight rows in flight)
    for (int y = y1 - 1; y >= y0; --y) {
      const int k = key(y);
      cnt = k == pk ? min(cnt + 1, d) : 0;
      pk = k;
      if (k && cnt >= d) down |= 1ull << (y - y0);
    }
  }
  const int kt = key(y0);
  int up = 0;
  if (kt)
    for (int y = y0 - 1; y >= 0 && up < d && key(y) == kt; --y) ++up;
  int pk = kt, cnt = up - 1;
#pragma unroll 8
  for (int y = y0; y < y1; ++y) {
    const size_t q = img + (size_t)y * W;
    const int L = labels[q];
    const int k = ((rowok[q] != 0) & (L > 0)) ? L : 0;
    cnt = k == pk ? min(cnt + 1, d) : 0;
    pk = k;
    const bool interior = k && cnt >= d && ((down >> (y - y0)) & 1ull);
    out[q] = (L > 0 && !interior) ? L : 0;
  }
}

// The smaller of the mask IoU i / u and the boundary IoU ib / ub of ground-truth id g, as a candidate: 0 / 1 when ub is 0, the mask
// fraction when they are equal.  Every factor is at most 2^27.
__device__ __forceinline__ ImCand bd_cand(int i, int u, int ib, int ub, int g) {
  if (ub == 0) return ImCand{0, 1, g};
  return (long long)i * ub <= (long long)ib * u ? ImCand{i, u, g} : ImCand{ib, ub, g};
}

// grid (thresholds + row blocks, images): im_match_kernel under the combined IoU.  Thread t owns ground-truth ids t + 1, t + 1 + NT, ...
// The blocks past the thresholds' write, one wave per predicted id, the ground-truth id of highest combined IoU with the two
// intersections (fields 2, 3, 5 of pred_rows); the first of them also counts the ids in use, from the mask table's areas.
__global__ __launch_bounds__(NT) void bd_match_kernel(const int* __restrict__ inter, const int* __restrict__ inter_bd, int P, int G, ImThresholds thr, int T,
                                                      const int* __restrict__ area_p, const int* __restrict__ area_g, const int* __restrict__ bd_area_p,
                                                      const int* __restrict__ bd_area_g, const int* __restrict__ rank, int* __restrict__ match,
                                                      int* __restrict__ gt_match, int* __restrict__ pred_rows, int* __restrict__ counts) {
  __shared__ int ap[MAX_IDS + 1], ag[MAX_IDS + 1], bp[MAX_IDS + 1], bg[MAX_IDS + 1], taken[MAX_IDS + 1];
  __shared__ int order[MAX_IDS];                                   // order[r] = the predicted id of rank r
  __shared__ ImCand wbest[2][WAVES];
  __shared__ int used[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = blockIdx.x, n = blockIdx.y;
  const size_t table = (size_t)n * (P + 1) * (G + 1);
  const int* cells = inter + table;
  const int* bcells = inter_bd + table;
  for (int p = tid; p <= P; p += NT) { ap[p] = area_p[(size_t)n * (P + 1) + p]; bp[p] = bd_area_p[(size_t)n * (P + 1) + p]; }
  for (int g = tid; g <= G; g += NT) { ag[g] = area_g[(size_t)n * (G + 1) + g]; bg[g] = bd_area_g[(size_t)n * (G + 1) + g]; taken[g] = 0; }
  if (k < T)
    for (int p = tid; p < P; p += NT) order[rank[(size_t)n * P + p]] = p + 1;    // (rank is a permutation of 0 .. P - 1)
  if (tid < 2) used[tid] = 0;
  __syncthreads();
  if (k >= T) {                                                    // (the whole block)
    const int e = k - T, E = gridDim.x - T;
    int* rows = pred_rows + (size_t)n * P * CAMO_BD_ROW_FIELDS;
    for (int p = e * WAVES + wave + 1; p <= P; p += E * WAVES) {
      const int a = ap[p], b = bp[p];
      const int* row = cells + (size_t)p * (G + 1);
      const int* brow = bcells + (size_t)p * (G + 1);
      ImCand best{0, 1, 0};
      if (a)
        for (int g = lane + 1; g <= G; g += 64) {
          const int i = row[g];
          if (i <= 0) continue;
          const int ib = brow[g];
          const ImCand c = bd_cand(i, a + ag[g] - i, ib, b + bg[g] - ib, g);
          if (im_before(c, best)) best = c;
        }
      best = im_wave_best(best);
      if (lane == 0) {
        rows[(size_t)(p - 1) * CAMO_BD_ROW_FIELDS + 2] = best.g;
        rows[(size_t)(p - 1) * CAMO_BD_ROW_FIELDS + 3] = best.g ? row[best.g] : 0;
        rows[(size_t)(p - 1) * CAMO_BD_ROW_FIELDS + 5] = best.g ? brow[best.g] : 0;
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
    if (tid < 2) counts[CAMO_IM_COUNTS * n + 2 + tid] = used[tid];
    return;
  }

  const long long num = thr.num[k], den = thr.den;
  int* mrow = match + ((size_t)n * T + k) * P;
  int buf = 0;
  for (int r = 0; r < P; ++r) {
    const int p = order[r], a = ap[p], b = bp[p];
    if (a == 0) {                                                  // (the whole block: no barrier is skipped by a part of it)
      if (tid == 0) mrow[p - 1] = 0;
      continue;
    }
    const int* row = cells + (size_t)p * (G + 1);
    const int* brow = bcells + (size_t)p * (G + 1);
    ImCand best{0, 1, 0};
    for (int g = tid + 1; g <= G; g += NT) {
      const int ga = ag[g];
      if (ga == 0 || taken[g]) continue;
      const int i = row[g];
      if (i <= 0) continue;
      const int ib = brow[g];
      const ImCand c = bd_cand(i, a + ga - i, ib, b + bg[g] - ib, g);
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

}  // namespace

int launch_boundary_labels(const int* labels, int N, int H, int W, int d, int* out, unsigned char* rowok, hipStream_t stream) {
  const bool none = 2ll * d + 1 > H || 2ll * d + 1 > W;            // the window is larger than the image: every foreground pixel is boundary
  if (!none) hipLaunchKernelGGL(bd_row_kernel, dim3((H + WAVES - 1) / WAVES, N), dim3(NT), 0, stream, labels, H, W, d, rowok);
  hipLaunchKernelGGL(bd_col_kernel, dim3((W + NT - 1) / NT, (H + STRIP - 1) / STRIP, N), dim3(NT), 0, stream, labels,
                     none ? nullptr : rowok, H, W, d, out);
  return (int)hipGetLastError();
}

BdWs bd_carve(int N, int P, int G, void* base) {
  BdWs w{};
  camo_abi::Carver c(base);
  w.area_p = c.take<int>((size_t)N * (P + 1));
  w.area_g = c.take<int>((size_t)N * (G + 1));
  w.rank = c.take<int>((size_t)N * P);
  w.bd_area_p = c.take<int>((size_t)N * (P + 1));
  w.bd_area_g = c.take<int>((size_t)N * (G + 1));
  w.bd_counts = c.take<int>((size_t)N * CAMO_IM_COUNTS);
  w.bytes = c.bytes();
  return w;
}

int launch_boundary_match(const int* pred_labels, const int* gt_labels, const int* pred_bd, const int* gt_bd, int N, int H, int W, int P, int G,
                          const long long* pred_table, int pred_table_rows, const ImThresholds& thr, int T, const BdWs& ws, int* inter,
                          int* inter_bd, int* pred_rows, int* gt_area, int* match, int* gt_match, int* counts, hipStream_t stream) {
  // the mask table: areas to fields 0 of pred_rows and gt_area, ranks to field 1; the boundary table: areas to fields 4 and 1
  if (int e = launch_im_table(pred_labels, gt_labels, N, H, W, P, G, pred_table, pred_table_rows, true, ws.area_p, ws.area_g, ws.rank, inter, pred_rows,
                              CAMO_BD_ROW_FIELDS, gt_area, CAMO_BD_GT_FIELDS, counts, stream))
    return e;
  if (int e = launch_im_table(pred_bd, gt_bd, N, H, W, P, G, nullptr, 0, false, ws.bd_area_p, ws.bd_area_g, nullptr, inter_bd, pred_rows + 4,
                              CAMO_BD_ROW_FIELDS, gt_area + 1, CAMO_BD_GT_FIELDS, ws.bd_counts, stream))
    return e;
  const int best_blocks = std::min((P + WAVES - 1) / WAVES, 16);
  hipLaunchKernelGGL(bd_match_kernel, dim3(T + best_blocks, N), dim3(NT), 0, stream, inter, inter_bd, P, G, thr, T, ws.area_p, ws.area_g, ws.bd_area_p,
                     ws.bd_area_g, ws.rank, match, gt_match, pred_rows, counts);
  return (int)hipGetLastError();
}
