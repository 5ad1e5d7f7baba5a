// Boundary IoU (include/camo_boundary.h): the boundary region of every instance of a label map -- the instance minus
// its erosion by a (2d + 1)^2 square, the image border counting as outside.  The erosion is separable and runs on runs of equal
// labels, so its cost does not follow d:
//
//   row     one wave per image row, 64 pixels a step: the run of equal labels a pixel is in, from two ballots, carried from step to step
//           along the row and never past its end; rowok = the run reaches d to the left and d to the right; one byte per pixel
//   column  one thread per column of a strip of BD_STRIP rows: over the key (the label where rowok, else none) the run of equal keys
//           must reach d up and d down; one sweep up the strip leaves a bit per row, one sweep down writes out
//
// The match under min(mask IoU, boundary IoU) of the maps this makes is inst_match.hip's.  Integer arithmetic only.
#include <hip/hip_runtime.h>

#include "boundary.h"
#include "common.h"
#include "label_inl.h"
#include "../../include/camo_boundary.h"

namespace {

constexpr int NT = BD_NT, WAVES = NT / 64, STRIP = BD_STRIP;
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

}  // namespace

int launch_boundary_labels(const int* labels, int N, int H, int W, int d, int* out, unsigned char* rowok, hipStream_t stream) {
  const bool none = 2ll * d + 1 > H || 2ll * d + 1 > W;            // the window is larger than the image: every foreground pixel is boundary
  if (!none) hipLaunchKernelGGL(bd_row_kernel, dim3((H + WAVES - 1) / WAVES, N), dim3(NT), 0, stream, labels, H, W, d, rowok);
  hipLaunchKernelGGL(bd_col_kernel, dim3((W + NT - 1) / NT, (H + STRIP - 1) / STRIP, N), dim3(NT), 0, stream, labels,
                     none ? nullptr : rowok, H, W, d, out);
  return (int)hipGetLastError();
}
