// Low-dynamic cores merged (include/camo_split_merge.h): a post-pass on the part map of either growth of the
// instance splitter.  A part whose best contact with a higher part is at least (num / den)^2 of its own peak, in squared distance,
// is linked to that part; the trees of the links are the new instances.  Every grid covers the whole batch; the launches do not
// depend on N or on the content.
//
//   column   per column the nearest background row of every pixel (split_inl.h's column_nearest); the first block of an image
//            clears its per-part arrays
//   d2       one block per image row: D2 in place (split_inl.h's row_distance2); peak[part] and owner[part] by integer max through
//            LDS tables of the row block; a foreground pixel whose part is out of range flags the image
//   pass     chunks of 1024 pixels: a pixel looks at its E, SW, S and SE neighbours, so every unordered contact is seen once, and
//            offers (value << 11 | 2047 - higher part) to the lower part's slot by 64-bit atomicMax; a run of equal slots over
//            consecutive lanes is reduced in the wave and is one atomic
//   groups   one block per image: the link test, the up pointers in LDS, 11 rounds of pointer jumping (2^11 > 1024 parts), the
//            smallest member of every root, the representatives ranked (label_compact): the new id of every part; counts
//   relabel  out_labels; the image's table rows cleared
//   table    the rows of the table from out_labels (split_inl.h's table_rows, inst_emit_inl.h)
//
// The image's per-part arrays hold CAMO_IM_MAX_IDS + 1 entries.  Integer atomics only: add, min, max, and the compare-and-swap of
// the table's LDS slots.  No block waits for another; every loop is bounded by the sizes.
#include <hip/hip_runtime.h>

#include "abi_util.h"
#include "split_inl.h"
#include "../../include/camo_split_merge.h"

namespace {

constexpr int JUMPS = 11, PER = (IDS + NT - 1) / NT;
static_assert((1 << JUMPS) >= IDS && IDS - 1 <= 2047 && 2ll * (SIDE - 1) * (SIDE - 1) < (1ll << 40), "a chain of every part; a part and a value in one key");
static_assert((long long)CAMO_SPLIT_MAX_DEN * CAMO_SPLIT_MAX_DEN * 2 * SIDE * SIDE < (1ll << 62), "the link test is 64-bit");

// a part value as an index of the per-part arrays: 0 when it is outside 1 .. CAMO_IM_MAX_IDS
__device__ __forceinline__ int merge_part(int v) { return (unsigned)(v - 1) < (unsigned)(IDS - 1) ? v : 0; }

// grid (ceil(W / COL_X), N): per column the nearest background row of every pixel.  An image's first block clears its per-part arrays.
__global__ __launch_bounds__(NT) void merge_column_kernel(const int* __restrict__ labels, int H, int W, int* __restrict__ ny, int* __restrict__ peak,
                                                          int* __restrict__ owner, unsigned long long* __restrict__ pass, int* __restrict__ bad) {
  const int n = blockIdx.y, tid = threadIdx.x, x = blockIdx.x * COL_X + tid % COL_X;
  if (blockIdx.x == 0) {
    for (int i = tid; i < IDS; i += NT) { peak[(size_t)n * PAD + i] = 0; owner[(size_t)n * PAD + i] = 0; pass[(size_t)n * PAD + i] = 0ull; }
    if (tid == 0) bad[n] = 0;
  }
  const int* g = labels + (size_t)n * H * W + min(x, W - 1);
  column_nearest(H, W, x < W, [&](int y) { return split_id(g[(size_t)y * W]) == 0; }, ny + (size_t)n * H * W + min(x, W - 1));
}

// grid (H, N): a block takes one row and overwrites it in place with D2 (0 on background, -1 when the image has no background).
// top[part] = the row's largest D2 + 2 (so that a part with a pixel is never 0) and own[part] = its largest id, added to peak and
// owner once per block and part.
__global__ __launch_bounds__(NT) void merge_d2_kernel(const int* __restrict__ labels, const int* __restrict__ parts, int H, int W, int* __restrict__ d2,
                                                      int* __restrict__ peak, int* __restrict__ owner, int* __restrict__ bad) {
  __shared__ int row[SIDE];
  __shared__ int top[IDS];
  __shared__ int own[IDS];
  const int n = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
  const int* lab = labels + ((size_t)n * H + y) * W;
  const int* prt = parts + ((size_t)n * H + y) * W;
  int* d = d2 + ((size_t)n * H + y) * W;
  for (int x = tid; x < W; x += NT) row[x] = d[x];
  for (int i = tid; i < IDS; i += NT) { top[i] = 0; own[i] = 0; }
  __syncthreads();
  int outside = 0;
  for (int x = tid; x < W; x += NT) {
    const int id = split_id(lab[x]);
    int best = 0;
    if (id) {
      best = row_distance2(row, W, x, y);
      const int a = merge_part(prt[x]);
      if (a) {
        if (top[a] < best + 2) atomicMax(&top[a], best + 2);
        if (own[a] < id) atomicMax(&own[a], id);
      } else {
        outside = 1;
      }
    }
    d[x] = best;
  }
  if (__syncthreads_or(outside) && tid == 0) atomicMax(bad + n, 1);
  for (int i = tid; i < IDS; i += NT)
    if (top[i]) { atomicMax(peak + (size_t)n * PAD + i, top[i]); atomicMax(owner + (size_t)n * PAD + i, own[i]); }
}

// grid (chunks, images).  A contact is a pair of 8-neighbours of one id in two parts a != b; b is higher than a when its peak is
// larger, or equal with b < a.  The lower part's slot takes the largest (min of the two D2 << 11 | 2047 - higher part): the best
// value, a tie to the smaller part.  An image with no background has D2 = -1 everywhere and offers nothing.
__global__ __launch_bounds__(NT) void merge_pass_kernel(const int* __restrict__ labels, const int* __restrict__ parts, const int* __restrict__ d2,
                                                        const int* __restrict__ peak, const int* __restrict__ bad, int H, int W,
                                                        unsigned long long* __restrict__ pass) {
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y, HW = H * W;
  if (bad[n]) return;                                              // (the whole block)
  const size_t base = (size_t)n * HW;
  const int* lab = labels + base;
  const int* prt = parts + base;
  const int* dd = d2 + base;
  const int* pk = peak + (size_t)n * PAD;
  unsigned long long* slot = pass + (size_t)n * PAD;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    int id = 0, a = 0, dp = 0, y = 0, x = 0;
    if (q < HW) {
      y = q / W; x = q - y * W;
      id = split_id(lab[q]);
      if (id) { a = merge_part(prt[q]); dp = dd[q]; }
      if (dp <= 0) a = 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int dy = k ? 1 : 0, dx = k ? k - 2 : 1;                // E, SW, S, SE
      int lower = 0;
      unsigned long long key = 0ull;
      if (a && y + dy < H && (unsigned)(x + dx) < (unsigned)W) {
        const int r = q + dy * W + dx;
        const int b = merge_part(prt[r]);
        if (b && b != a && split_id(lab[r]) == id) {
          const int v = min(dp, dd[r]), pa = pk[a], pb = pk[b];
          const bool b_higher = pb > pa || (pb == pa && b < a);
          lower = b_higher ? a : b;
          key = ((unsigned long long)v << 11) | (unsigned long long)(2047 - (b_higher ? b : a));
        }
      }
      if (__ballot(lower != 0) == 0ull) continue;                  // (wave-uniform)
      const int prev = __shfl_up(lower, 1, 64);
      const bool head = lane == 0 || prev != lower;
      const int end = run_end(head, lane);
      for (int s = 1; s < 64; s <<= 1) {                           // the run's largest key reaches its head
        const unsigned long long other = __shfl_down(key, s, 64);
        if (lane + s < end && other > key) key = other;
      }
      if (head && lower) atomicMax(slot + lower, key);
    }
  }
}

// One block per image.  up[a] = the part a is linked to, a itself when it is not; after the jumps the root of its group.
__global__ __launch_bounds__(NT) void merge_groups_kernel(const unsigned long long* __restrict__ pass, const int* __restrict__ peak,
                                                          const int* __restrict__ owner, const int* __restrict__ bad, long long num2, long long den2,
                                                          int* __restrict__ new_id, int* __restrict__ counts) {
  __shared__ int up[IDS], first[IDS], members[IDS], rank[IDS], owned[IDS], lo[IDS], hi[IDS];
  __shared__ int wcount[NT / 64];
  __shared__ int tally[3];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (bad[n]) {                                                    // (the whole block)
    if (tid < 4) counts[4 * n + tid] = tid ? 0 : -1;
    return;
  }
  const int* pk = peak + (size_t)n * PAD;
  for (int a = tid; a < IDS; a += NT) {
    int u = a;
    const int p = a ? pk[a] : 0;
    const unsigned long long key = p > 0 ? pass[(size_t)n * PAD + a] : 0ull;
    if (key && den2 * (long long)(key >> 11) >= num2 * (long long)(p - 2)) u = min(2047 - (int)(key & 2047ull), IDS - 1);      // (a key names a part)
    up[a] = u; first[a] = FAR; members[a] = 0; rank[a] = 0; owned[a] = 0; lo[a] = FAR; hi[a] = 0;
  }
  if (tid < 3) tally[tid] = 0;
  __syncthreads();
  for (int round = 0; round < JUMPS; ++round) {
    int next[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) { const int a = i * NT + tid; next[i] = a < IDS ? up[up[a]] : 0; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) { const int a = i * NT + tid; if (a < IDS) up[a] = next[i]; }
    __syncthreads();
  }
  for (int a = tid; a < IDS; a += NT) {
    if (a == 0 || pk[a] <= 0) continue;
    const int r = up[a], o = owner[(size_t)n * PAD + a];
    atomicMin(&first[r], a); atomicAdd(&members[r], 1);
    atomicAdd(&owned[o], 1); atomicMin(&lo[o], r); atomicMax(&hi[o], r);
  }
  __syncthreads();
  const int groups = label_compact<NT>(IDS, wcount, [&](int r) { return r > 0 && pk[r] > 0 && first[up[r]] == r; },
                                       [&](int r, int before) { if (before >= 0) rank[up[r]] = before + 1; });
  __syncthreads();
  int present = 0, joined = 0, whole = 0;
  for (int a = tid; a < IDS; a += NT) {
    const bool here = a > 0 && pk[a] > 0;
    new_id[(size_t)n * PAD + a] = here ? rank[up[a]] : 0;
    present += here; joined += members[a] >= 2; whole += owned[a] >= 2 && lo[a] == hi[a];
  }
  present = wave_sum_int(present); joined = wave_sum_int(joined); whole = wave_sum_int(whole);
  if (lane == 0) { atomicAdd(&tally[0], present); atomicAdd(&tally[1], joined); atomicAdd(&tally[2], whole); }
  __syncthreads();
  if (tid == 0) { counts[4 * n] = groups; counts[4 * n + 1] = tally[0]; counts[4 * n + 2] = tally[1]; counts[4 * n + 3] = tally[2]; }
}

// grid (chunks, images): out = the new id of the pixel's part, the part value itself in an image that is not supported, 0 where
// labels reads 0; the image's table rows cleared.
__global__ __launch_bounds__(NT) void merge_relabel_kernel(const int* __restrict__ labels, const int* __restrict__ parts, const int* __restrict__ new_id,
                                                           const int* __restrict__ bad, const int* __restrict__ counts, int H, int W, int max_instances,
                                                           int* __restrict__ out, unsigned long long* __restrict__ table) {
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  emit_clear_rows<NT>(table + (size_t)n * max_instances * 8, counts[4 * n], max_instances);
  const bool as_given = bad[n] != 0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    if (q >= HW) continue;
    const int id = split_id(labels[base + q]), v = parts[base + q];
    out[base + q] = id ? (as_given ? v : new_id[(size_t)n * PAD + merge_part(v)]) : 0;
  }
}

// grid (chunks, images): the table's rows from out; an image that is not supported keeps its cleared rows
__global__ __launch_bounds__(NT) void merge_table_kernel(const float* __restrict__ pred, long long stride, const int* __restrict__ out,
                                                         const int* __restrict__ bad, int H, int W, int max_instances,
                                                         unsigned long long* __restrict__ table) {
  __shared__ EmitSlots slots;
  if (bad[blockIdx.y]) return;                                     // (the whole block)
  table_rows(slots, pred, stride, out, H, W, max_instances, table);
}

}  // namespace

SplitMergeWs split_merge_carve(int N, int H, int W, void* base) {
  SplitMergeWs w{};
  camo_abi::Carver c(base);
  w.d2 = c.take<int>((size_t)N * H * W);
  w.pass = c.take<unsigned long long>((size_t)N * PAD);
  w.peak = c.take<int>((size_t)N * PAD);
  w.owner = c.take<int>((size_t)N * PAD);
  w.new_id = c.take<int>((size_t)N * PAD);
  w.bad = c.take<int>((size_t)N);
  w.bytes = c.bytes();
  return w;
}

int launch_split_merge(const int* labels, const int* parts, const float* pred, long long stride, int N, int H, int W, int num, int den,
                       int max_instances, const SplitMergeWs& ws, int* out, long long* table, int* counts, hipStream_t stream) {
  const int chunks = (int)(((long long)H * W + CHUNK - 1) / CHUNK), cols = (W + COL_X - 1) / COL_X;
  const dim3 raster(chunks, N);
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table);
  hipLaunchKernelGGL(merge_column_kernel, dim3(cols, N), dim3(NT), 0, stream, labels, H, W, ws.d2, ws.peak, ws.owner, ws.pass, ws.bad);
  hipLaunchKernelGGL(merge_d2_kernel, dim3(H, N), dim3(NT), 0, stream, labels, parts, H, W, ws.d2, ws.peak, ws.owner, ws.bad);
  hipLaunchKernelGGL(merge_pass_kernel, raster, dim3(NT), 0, stream, labels, parts, ws.d2, ws.peak, ws.bad, H, W, ws.pass);
  hipLaunchKernelGGL(merge_groups_kernel, dim3(N), dim3(NT), 0, stream, ws.pass, ws.peak, ws.owner, ws.bad, (long long)num * num, (long long)den * den,
                     ws.new_id, counts);
  hipLaunchKernelGGL(merge_relabel_kernel, raster, dim3(NT), 0, stream, labels, parts, ws.new_id, ws.bad, counts, H, W, max_instances, out, tab);
  hipLaunchKernelGGL(merge_table_kernel, raster, dim3(NT), 0, stream, pred, stride, out, ws.bad, H, W, max_instances, tab);
  return (int)hipGetLastError();
}
