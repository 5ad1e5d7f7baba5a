// Object instances of a predicted mask (include/camo_instances.h): binarise, fill holes, label the connected
// components, drop the small ones, number the rest in reading order, and sum (area, box, Sx, Sy, Sq) per component.  4 B/pixel in
// and 5 B/pixel out: the work is launches and latency, so every grid covers the whole batch.
//
//   label tiles  one block per 32 x 32 tile: membership of each pixel (background for the hole pass; foreground, or foreground and
//                holes, for the component pass), then the components of the tile's members in LDS (cc_inl.h): every member points
//                at the smallest index of its component inside the tile
//   join tiles   members on a tile border: cc_inl.h's unions with their neighbours in other tiles, on the global parents
//   flatten      every member finds its root and points at it.  Hole pass: a member on the image's border sets border[root].
//                Component pass: area[root] += 1, runs of equal root combined in the wave and the block's first root in the block
//   count        per chunk of 1024 pixels: the kept roots, the dropped roots, the pixels of the kept
//   scan         one block per image: the chunks' exclusive prefix of kept roots; counts
//   rank         id[root] = the prefix + the kept roots before it in the chunk + 1 (0 when dropped); the image's table rows cleared
//   emit         labels, clean, and the table's sums, minima and maxima, through a block's LDS slots (inst_emit_inl.h)
//
// With fill_holes the first three run twice: on the background with the complementary connectivity, then on the filled foreground.
// Union by atomicMin on the larger root (cc_inl.h): the output depends on the partition alone.  Integer atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "cc_inl.h"
#include "common.h"
#include "inst_emit_inl.h"
#include "instances.h"
#include "label_inl.h"

namespace {

constexpr int T = INST_TILE, NT = INST_NT, CHUNK = INST_CHUNK, PPT = INST_CHUNK / INST_NT;
constexpr int MODE_BG = 0, MODE_FG = 1, MODE_FILLED = 2;
constexpr int NONE = 0x7fffffff;
static_assert(T * T % NT == 0 && CHUNK % NT == 0 && NT % 64 == 0, "whole waves, whole passes");

// grid (tiles of an image, images; an image loop when the grid would be too large).  MODE_BG: members are the background pixels,
// border[] is cleared.  MODE_FG: members are the foreground pixels.  MODE_FILLED: the foreground pixels and those of the background
// components (bgpar, flattened) that do not touch the border; a root of such a component counts one hole.  The component modes clear area[].
template <int CONN, int MODE>
__global__ __launch_bounds__(NT) void inst_label_tiles_kernel(const float* __restrict__ pred, long long stride, float threshold, int N, int H, int W,
                                                              int tiles_x, const int* __restrict__ bgpar, unsigned char* border,
                                                              int* __restrict__ par, int* __restrict__ area, int* __restrict__ misc) {
  __shared__ int lab[T * T];
  __shared__ int holes;
  const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, y0 = ty * T, x0 = tx * T;
  const size_t HW = (size_t)H * W;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const size_t base = (size_t)n * HW;
    const float* img = pred + (size_t)n * stride;
    if (tid == 0) {
      holes = 0;
      if (MODE != MODE_FILLED && blockIdx.x == 0) misc[n] = 0;      // (MODE_FILLED adds to what the hole pass's launch cleared)
    }
    __syncthreads();
    int nh = 0;
    for (int l = tid; l < T * T; l += NT) {
      const int y = y0 + l / T, x = x0 + l % T;
      bool member = false;
      if (y < H && x < W) {
        const size_t q = (size_t)y * W + x, p = base + q;
        const bool fg = img[q] > threshold;                          // (a NaN compares false: background)
        if (MODE == MODE_BG) {
          member = !fg;
          border[p] = 0;
        } else {
          member = fg;
          if (MODE == MODE_FILLED && !fg) {
            const int r = bgpar[p];                                  // (flattened: the root)
            member = !border[r];
            if (member && r == (int)p) ++nh;
          }
          area[p] = 0;
        }
      }
      lab[l] = cc_run_parent<T, NT>(l, member, cc_all{});
    }
    if (MODE == MODE_FILLED && nh) atomicAdd(&holes, nh);
    __syncthreads();
    for (int l = tid; l < T * T; l += NT) cc_tile_unions<CONN, T>(lab, l, cc_all{});
    __syncthreads();
    for (int l = tid; l < T * T; l += NT) {
      const int y = y0 + l / T, x = x0 + l % T;
      if (y >= H || x >= W) continue;
      par[base + (size_t)y * W + x] = lab[l] >= 0 ? cc_tile_root<T>(lab, l, base, y0, x0, W) : -1;
    }
    if (MODE == MODE_FILLED && tid == 0 && holes) atomicAdd(misc + n, holes);
    __syncthreads();                                                 // lab and holes are reused by the next image
  }
}

template <int CONN>
__global__ __launch_bounds__(NT) void inst_join_tiles_kernel(int* par, int N, int H, int W) {
  const long long total = (long long)N * H * W, p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  // (a member's parent was written by the launch before and stays >= 0)
  cc_join_borders<CONN, T>(par, p, H, W, [par](long long q) { return par[q] >= 0; }, cc_all{});
}

// hole pass: every background pixel points at its root; one on the image's border marks the root
__global__ __launch_bounds__(NT) void inst_flatten_bg_kernel(int* par, unsigned char* border, int N, int H, int W) {
  const long long total = (long long)N * H * W, p = (long long)blockIdx.x * NT + threadIdx.x;
  if (p >= total) return;
  if (par[p] < 0) return;
  const int r = cc_flatten(par, p);
  const int q = (int)(p % ((long long)H * W)), y = q / W, x = q - y * W;
  if (y == 0 || y == H - 1 || x == 0 || x == W - 1) border[r] = 1;      // (every writer stores the same byte)
}

// grid (chunks, images).  Component pass: every member points at its root, area[root] counts it.  The block's smallest root is
// counted in LDS and added once; every other run of equal roots over consecutive lanes is one atomic.
__global__ __launch_bounds__(NT) void inst_flatten_area_kernel(int* par, int* __restrict__ area, int H, int W) {
  __shared__ int dom, dom_count;
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  if (tid == 0) { dom = NONE; dom_count = 0; }
  __syncthreads();
  int r[PPT], mine = NONE;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    r[j] = -1;
    if (q < HW) {
      const size_t p = base + q;
      if (par[p] >= 0) {
        r[j] = cc_flatten(par, (long long)p);
        mine = min(mine, r[j]);
      }
    }
  }
  mine = wave_min_int(mine);
  if (lane == 0 && mine != NONE) atomicMin(&dom, mine);
  __syncthreads();
  const int d = dom;
  if (d == NONE) return;                                          // (the whole block: no member in the chunk)
  int nd = 0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    nd += r[j] == d;
    const int key = r[j] == d ? -1 : r[j];
    if (__ballot(key >= 0) == 0ull) continue;                     // (wave-uniform)
    const int prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const int end = run_end(head, lane);
    if (head && key >= 0) atomicAdd(area + key, end - lane);
  }
  nd = wave_sum_int(nd);
  if (lane == 0 && nd) atomicAdd(&dom_count, nd);
  __syncthreads();
  if (tid == 0) atomicAdd(area + d, dom_count);
}

// grid (chunks, images): chunk[0] = roots of at least min_area pixels, chunk[1] = smaller roots, chunk[2] = pixels of the former
__global__ __launch_bounds__(NT) void inst_count_kernel(const int* __restrict__ par, const int* __restrict__ area, int H, int W, int min_area,
                                                        int N, int* __restrict__ chunk) {
  __shared__ int s[3];
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  if (tid < 3) s[tid] = 0;
  __syncthreads();
  int nk = 0, ns = 0, np = 0;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    if (q >= HW) continue;
    const size_t p = base + q;
    if (par[p] != (int)p) continue;
    const int a = area[p];
    if (a >= min_area) { ++nk; np += a; } else ++ns;
  }
  nk = wave_sum_int(nk); ns = wave_sum_int(ns); np = wave_sum_int(np);
  if (lane == 0) {
    if (nk) { atomicAdd(&s[0], nk); atomicAdd(&s[2], np); }
    if (ns) atomicAdd(&s[1], ns);
  }
  __syncthreads();
  if (tid < 3) chunk[((size_t)tid * N + n) * gridDim.x + blockIdx.x] = s[tid];
}

// one block per image: chunk[0] becomes its exclusive prefix; counts = {kept, dropped, holes, pixels of the kept}
__global__ __launch_bounds__(NT) void inst_scan_kernel(int* __restrict__ chunk, int chunks, int N, const int* __restrict__ misc,
                                                       int* __restrict__ counts) {
  __shared__ int s[NT];
  __shared__ int tot[2];
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.x;
  const int* cs = chunk + ((size_t)N + n) * chunks;
  const int* cp = chunk + ((size_t)2 * N + n) * chunks;
  if (tid < 2) tot[tid] = 0;
  int ns = 0, np = 0;
  const int kept = block_chunk_prefix<NT>(chunk + (size_t)n * chunks, chunks, s, [&](int i) { ns += cs[i]; np += cp[i]; });
  ns = wave_sum_int(ns); np = wave_sum_int(np);
  if (lane == 0) { atomicAdd(&tot[0], ns); atomicAdd(&tot[1], np); }
  __syncthreads();
  if (tid == 0) { counts[4 * n] = kept; counts[4 * n + 1] = tot[0]; counts[4 * n + 2] = misc[n]; counts[4 * n + 3] = tot[1]; }
}

// grid (chunks, images): rid[root] = the component's id, 0 when it is dropped.  The image's table rows are cleared on the way, the
// box minima of the rows in use to the largest value.
__global__ __launch_bounds__(NT) void inst_rank_kernel(const int* __restrict__ par, const int* __restrict__ area, int H, int W, int min_area,
                                                       const int* __restrict__ chunk, const int* __restrict__ counts, int max_instances,
                                                       int* __restrict__ rid, unsigned long long* __restrict__ table) {
  __shared__ int wcount[NT / 64];
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  emit_clear_rows<NT>(table + (size_t)n * max_instances * 8, counts[4 * n], max_instances);
  int running = chunk[(size_t)n * gridDim.x + blockIdx.x];
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    const size_t p = base + q;
    const bool root = q < HW && par[p] == (int)p;
    const bool kept = root && area[p] >= min_area;
    int total;
    const int before = block_rank<NT>(kept, wcount, total);
    if (root) rid[p] = kept ? running + before + 1 : 0;
    running += total;
    __syncthreads();
  }
}

// grid (chunks, images).  labels and clean of every pixel, and the table through inst_emit_inl.h's run records and LDS slots.
__global__ __launch_bounds__(NT) void inst_emit_kernel(const float* __restrict__ pred, long long stride, const int* __restrict__ par,
                                                       const int* __restrict__ rid, int H, int W, int max_instances, int* __restrict__ labels,
                                                       unsigned char* __restrict__ clean, unsigned long long* __restrict__ table) {
  __shared__ EmitSlots slots;
  const int tid = threadIdx.x, n = blockIdx.y, HW = H * W;
  const size_t base = (size_t)n * HW;
  const float* img = pred + (size_t)n * stride;
  emit_slots_clear(slots);
  __syncthreads();
  unsigned long long* rows = table + (size_t)n * max_instances * 8;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int q = blockIdx.x * CHUNK + j * NT + tid;
    int k = 0;
    float pv = 0.f;
    if (q < HW) {
      const size_t p = base + q;
      pv = img[q];
      const int r = par[p];
      const int id = r >= 0 ? rid[r] : 0;
      labels[p] = id;
      clean[p] = id > 0 ? 1 : 0;
      if (id <= max_instances) k = id;                            // (ids past the table keep their label and have no row)
    }
    emit_record(slots, rows, k, q, W, quantise_u8(pv));
  }
  __syncthreads();
  emit_slots_flush(slots, rows);
}

unsigned blocks_of(long long count) { return (unsigned)((count + NT - 1) / NT); }

}  // namespace

InstWs inst_carve(int N, int H, int W, void* base) {
  InstWs w{};
  camo_abi::Carver c(base);
  const size_t npix = (size_t)N * H * W, chunks = ((size_t)H * W + CHUNK - 1) / CHUNK;
  w.bgpar = c.take<int>(npix);
  w.par = c.take<int>(npix);
  w.area = c.take<int>(npix);
  w.border = c.take<unsigned char>(npix);
  w.chunk = c.take<int>(3 * (size_t)N * chunks);
  w.misc = c.take<int>((size_t)N);
  w.bytes = c.bytes();
  return w;
}

template <int CONN, int MODE>
static void label_pass(const float* pred, long long stride, float threshold, int N, int H, int W, const InstWs& ws, int* par, hipStream_t stream) {
  const int tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
  const long long tiles = (long long)tiles_x * tiles_y;                      // <= 2^21 (H * W <= 2^26)
  // at most 2^32 - 1 threads in a grid: beyond that a block takes several images
  const int rows = (int)std::min<long long>(N, ((1ll << 32) - 1) / (tiles * NT));
  hipLaunchKernelGGL((inst_label_tiles_kernel<CONN, MODE>), dim3((unsigned)tiles, (unsigned)rows), dim3(NT), 0, stream, pred, stride, threshold, N, H,
                     W, tiles_x, ws.bgpar, ws.border, par, ws.area, ws.misc);
  hipLaunchKernelGGL(inst_join_tiles_kernel<CONN>, dim3(blocks_of((long long)N * H * W)), dim3(NT), 0, stream, par, N, H, W);
}

int launch_instances(const float* pred, long long stride, float threshold, int N, int H, int W, int connectivity, int min_area, bool fill_holes,
                     int max_instances, const InstWs& ws, int* labels, unsigned char* clean, long long* table, int* counts, hipStream_t stream) {
  const long long total = (long long)N * H * W;
  const int chunks = (int)(((long long)H * W + CHUNK - 1) / CHUNK);
  const dim3 raster(chunks, N);
  const bool eight = connectivity == 8;
  if (fill_holes) {
    if (eight) label_pass<4, MODE_BG>(pred, stride, threshold, N, H, W, ws, ws.bgpar, stream);
    else label_pass<8, MODE_BG>(pred, stride, threshold, N, H, W, ws, ws.bgpar, stream);
    hipLaunchKernelGGL(inst_flatten_bg_kernel, dim3(blocks_of(total)), dim3(NT), 0, stream, ws.bgpar, ws.border, N, H, W);
    if (eight) label_pass<8, MODE_FILLED>(pred, stride, threshold, N, H, W, ws, ws.par, stream);
    else label_pass<4, MODE_FILLED>(pred, stride, threshold, N, H, W, ws, ws.par, stream);
  } else {
    if (eight) label_pass<8, MODE_FG>(pred, stride, threshold, N, H, W, ws, ws.par, stream);
    else label_pass<4, MODE_FG>(pred, stride, threshold, N, H, W, ws, ws.par, stream);
  }
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table);
  hipLaunchKernelGGL(inst_flatten_area_kernel, raster, dim3(NT), 0, stream, ws.par, ws.area, H, W);
  hipLaunchKernelGGL(inst_count_kernel, raster, dim3(NT), 0, stream, ws.par, ws.area, H, W, min_area, N, ws.chunk);
  hipLaunchKernelGGL(inst_scan_kernel, dim3(N), dim3(NT), 0, stream, ws.chunk, chunks, N, ws.misc, counts);
  hipLaunchKernelGGL(inst_rank_kernel, raster, dim3(NT), 0, stream, ws.par, ws.area, H, W, min_area, ws.chunk, counts, max_instances, ws.bgpar, tab);
  hipLaunchKernelGGL(inst_emit_kernel, raster, dim3(NT), 0, stream, pred, stride, ws.par, ws.bgpar, H, W, max_instances, labels, clean, tab);
  return (int)hipGetLastError();
}
