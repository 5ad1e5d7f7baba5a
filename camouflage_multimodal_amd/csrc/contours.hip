// Instance contours (include/camo_contours.h): label maps to the closed rings of every id, vertices on pixel corners.
// Every grid covers the whole batch; no block waits for another.
//
//   count     per CT_CHUNK consecutive pixels: a pixel's 4-bit crack mask and its cracks' offset within the chunk, the chunk's count;
//             the blocks of an image also clear its rows of rings and xy
//   scan      one block per image: exclusive prefix of the chunk counts (label_inl.h's label_scan), E, cracks taken
//   link      per pixel: a crack's compact position, its successor's, its index, its successor's is-vertex bit
//   doubling  (LDS form) one block per image, the link state of every crack one 32-bit word in each of two LDS buffers: min-doubling
//             to the ring heads, then the weighted suffix doubling to every crack's vertices-to-the-end
//   head / place round   (global form) one round of either doubling, (value, next) pairs from one buffer into the other
//   rank      one block per image: heads ranked over compact order (label_compact), ring vertex counts scanned to offsets, rows, counts
//   emit      per crack: a vertex crack's corner to xy, every crack's a2 term to its ring (64-bit atomic add per run of equal ring in a wave)
//
// Integer arithmetic only; the one atomic is the 64-bit atomicAdd of emit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "abi_util.h"
#include "common.h"
#include "label_inl.h"
#include "contours.h"
#include "../../include/camo_contours.h"

namespace {

constexpr int NT = CT_CHUNK, WAVES = NT / 64;
constexpr int NTB = 1024;                              // threads of the kernels that run one block per image
constexpr int LDS_BYTES = 2 * CT_LDS_CRACKS * 4;      // two buffers of one word a crack
constexpr unsigned END = 0xFFFFu;                      // the low half of a cut chain's last crack: no position, positions are < 2^14
constexpr int NCOUNTS = CAMO_CONTOUR_COUNTS, TAKEN = 3, NFIELDS = CAMO_CONTOUR_RING_FIELDS;
static_assert(CT_LDS_CRACKS == CAMO_CONTOUR_LDS_CRACKS, "include/camo_contours.h states the kernel's constant");
static_assert(CT_LDS_CRACKS <= (1 << 15) && LDS_BYTES <= 160 * 1024, "two 16-bit halves a word, two words a crack, inside a CU's LDS");
static_assert(4 * (CT_CHUNK - 1) < (1 << 12), "a pixel's offset within its chunk and its mask share 16 bits");

// the heading of side s: (+1, 0), (0, +1), (-1, 0), (0, -1)
__device__ __forceinline__ int side_dx(int s) { return (s == 0) - (s == 2); }
__device__ __forceinline__ int side_dy(int s) { return (s == 1) - (s == 3); }

// the compact position of the crack on side s of pixel q (which has it): chunk prefix + offset in the chunk + the mask bits below s
__device__ __forceinline__ int crack_position(const unsigned short* __restrict__ pix, const int* __restrict__ pre, int q, int s) {
  const unsigned w = pix[q];
  return pre[q / NT] + (int)(w >> 4) + __popc(w & ((1u << s) - 1u));
}

// grid (chunks, images)
__global__ __launch_bounds__(NT) void ct_count_kernel(const int* __restrict__ labels, int H, int W, int chunks, int R, int V,
                                                      unsigned short* __restrict__ pix, int* __restrict__ cnt, long long* __restrict__ rings,
                                                      int* __restrict__ xy) {
  __shared__ int wsum[WAVES];
  const int n = blockIdx.y, HW = H * W, p = blockIdx.x * NT + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* img = labels + (size_t)n * HW;
  int mask = 0;
  if (p < HW) {
    const int y = p / W, x = p - y * W, L = img[p];
    if (L > 0)
      mask = (int)(y == 0 || img[p - W] != L) | ((int)(x == W - 1 || img[p + 1] != L) << 1) | ((int)(y == H - 1 || img[p + W] != L) << 2) |
             ((int)(x == 0 || img[p - 1] != L) << 3);
  }
  const int c = __popc(mask), inc = wave_scan_int(c);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int off = inc - c, total = 0;
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) off += wsum[w];
    total += wsum[w];
  }
  if (p < HW) pix[(size_t)n * HW + p] = (unsigned short)((off << 4) | mask);
  if (threadIdx.x == 0) cnt[(size_t)n * chunks + blockIdx.x] = total;
  const long long step = (long long)gridDim.x * NT, first = (long long)blockIdx.x * NT + threadIdx.x;      // the image's rows, shared among its blocks
  long long* rows = rings + (size_t)n * R * NFIELDS;
  for (long long i = first; i < (long long)R * NFIELDS; i += step) rows[i] = 0;
  int2* corners = reinterpret_cast<int2*>(xy) + (size_t)n * V;
  for (long long i = first; i < V; i += step) corners[i] = make_int2(0, 0);
}

// grid (images)
__global__ __launch_bounds__(NTB) void ct_scan_kernel(const int* __restrict__ cnt, int chunks, int C, int* __restrict__ pre, int* __restrict__ counts) {
  __shared__ int wsum[NTB / 64];
  const int n = blockIdx.x;
  const int E = label_scan<NTB>(cnt + (size_t)n * chunks, chunks, pre + (size_t)n * chunks, wsum);
  if (threadIdx.x == 0) {
    int* c = counts + (size_t)n * NCOUNTS;
    c[0] = E; c[1] = 0; c[2] = 0; c[TAKEN] = E <= C ? E : 0; c[4] = 0; c[5] = 0;      // (rank fills in the rings and vertices of an image that takes its cracks)
  }
}

// grid (chunks, images)
__global__ __launch_bounds__(NT) void ct_link_kernel(const int* __restrict__ labels, int H, int W, int chunks, int eight, int C,
                                                     const unsigned short* __restrict__ pix, const int* __restrict__ pre, const int* __restrict__ counts,
                                                     int* __restrict__ next, int* __restrict__ crack, unsigned char* __restrict__ vert) {
  const int n = blockIdx.y, HW = H * W, p = blockIdx.x * NT + threadIdx.x;
  const int taken = counts[(size_t)n * NCOUNTS + TAKEN];
  if (taken == 0 || p >= HW) return;                                 // (no cross-lane step follows)
  const unsigned short* px = pix + (size_t)n * HW;
  const int* pr = pre + (size_t)n * chunks;
  const int* img = labels + (size_t)n * HW;
  const unsigned w = px[p];
  const int mask = w & 15;
  if (mask == 0) return;
  const int y = p / W, x = p - y * W, L = img[p], base = pr[blockIdx.x] + (int)(w >> 4);
  const size_t at = (size_t)n * C;
  auto has = [&](int yy, int xx) { return yy >= 0 && yy < H && xx >= 0 && xx < W && img[yy * W + xx] == L; };
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (!((mask >> s) & 1)) continue;
    const int pos = base + __popc(mask & ((1 << s) - 1));
    const int dx = side_dx(s), dy = side_dy(s);
    const int bx = x + dx, by = y + dy, ax = bx + dy, ay = by - dx;      // b: after p along the heading; a: to the left of b
    const bool a = has(ay, ax), b = has(by, bx);
    int q = p, t = (s + 1) & 3;                                       // turn right
    if (a && (b || eight)) { q = ay * W + ax; t = (s + 3) & 3; }      // turn left
    else if (b) { q = by * W + bx; t = s; }                           // straight on
    int to = crack_position(px, pr, q, t);
    if (to >= taken) to = pos;                                        // (never: the successor is a crack of this image; keeps every later gather inside the arrays)
    else vert[at + to] = (unsigned char)(t != s);
    if (pos < taken) { next[at + pos] = to; crack[at + pos] = 4 * p + s; }
  }
}

// One block per image, dynamic LDS of LDS_BYTES: two buffers of one word a crack, word i = (value << 16) | next.  A round reads one
// buffer and writes the other, one barrier a round.  grid (images)
__global__ __launch_bounds__(NTB) void ct_doubling_kernel(const int* __restrict__ next, const unsigned char* __restrict__ vert, const int* __restrict__ counts,
                                                          int C, int2* __restrict__ head, int2* __restrict__ place) {
  extern __shared__ __align__(16) unsigned st[];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int E = counts[(size_t)n * NCOUNTS + TAKEN];
  if (E == 0) return;                                                // (the whole block)
  const size_t at = (size_t)n * C;
  unsigned *a = st, *b = st + CT_LDS_CRACKS;
  for (int i = tid; i < E; i += NTB) a[i] = ((unsigned)i << 16) | (unsigned)next[at + i];
  __syncthreads();
  for (int len = 1; len < E; len <<= 1) {                            // heads
    for (int i = tid; i < E; i += NTB) {
      const unsigned w = a[i], wj = a[w & 0xFFFFu];
      b[i] = (min(w >> 16, wj >> 16) << 16) | (wj & 0xFFFFu);
    }
    __syncthreads();
    unsigned* t = a; a = b; b = t;
  }
  for (int i = tid; i < E; i += NTB) {
    const unsigned h = a[i] >> 16, nx = (unsigned)next[at + i];
    head[at + i] = make_int2((int)h, 0);
    b[i] = ((unsigned)vert[at + i] << 16) | (nx == h ? END : nx);
  }
  __syncthreads();
  { unsigned* t = a; a = b; b = t; }
  for (int len = 1; len < E; len <<= 1) {                            // places
    for (int i = tid; i < E; i += NTB) {
      unsigned w = a[i];
      const unsigned j = w & 0xFFFFu;
      if (j != END) {
        const unsigned wj = a[j];
        w = (((w >> 16) + (wj >> 16)) << 16) | (wj & 0xFFFFu);
      }
      b[i] = w;
    }
    __syncthreads();
    unsigned* t = a; a = b; b = t;
  }
  for (int i = tid; i < E; i += NTB) place[at + i] = make_int2((int)(a[i] >> 16), 0);
}

// grid (crack blocks, images).  FIRST: the round reads the link pass's array, (m, next) = (own position, successor)
template <bool FIRST>
__global__ __launch_bounds__(NT) void ct_head_round_kernel(const int* __restrict__ next, const int2* __restrict__ in, int2* __restrict__ out,
                                                           const int* __restrict__ counts, int C) {
  const int n = blockIdx.y, i = blockIdx.x * NT + threadIdx.x;
  if (i >= counts[(size_t)n * NCOUNTS + TAKEN]) return;
  const size_t at = (size_t)n * C;
  const int2 a = FIRST ? make_int2(i, next[at + i]) : in[at + i];
  const int2 b = FIRST ? make_int2(a.y, next[at + a.y]) : in[at + a.y];
  out[at + i] = make_int2(min(a.x, b.x), b.y);
}

// grid (crack blocks, images).  FIRST: (s, next) = (is-vertex bit, successor or -1 where the successor is the ring's head)
template <bool FIRST>
__global__ __launch_bounds__(NT) void ct_place_round_kernel(const int* __restrict__ next, const unsigned char* __restrict__ vert, const int2* __restrict__ head,
                                                            const int2* __restrict__ in, int2* __restrict__ out, const int* __restrict__ counts, int C) {
  const int n = blockIdx.y, i = blockIdx.x * NT + threadIdx.x;
  if (i >= counts[(size_t)n * NCOUNTS + TAKEN]) return;
  const size_t at = (size_t)n * C;
  auto first = [&](int j) {
    const int nx = next[at + j];
    return make_int2((int)vert[at + j], nx == head[at + j].x ? -1 : nx);
  };
  int2 a = FIRST ? first(i) : in[at + i];
  if (a.y >= 0) {
    const int2 b = FIRST ? first(a.y) : in[at + a.y];
    a = make_int2(a.x + b.x, b.y);
  }
  out[at + i] = a;
}

// grid (images)
__global__ __launch_bounds__(NTB) void ct_rank_kernel(const int* __restrict__ labels, int HW, const int* __restrict__ crack, const int2* __restrict__ head,
                                                      const int2* __restrict__ place, int C, int R, int V, int* __restrict__ ring_of,
                                                      int* __restrict__ ring_head, int* __restrict__ ring_nv, int* __restrict__ ring_off,
                                                      long long* __restrict__ rings, int* __restrict__ counts) {
  __shared__ int wcount[NTB / 64];
  const int n = blockIdx.x;
  int* c = counts + (size_t)n * NCOUNTS;
  const int E = c[TAKEN];
  if (E == 0) return;                                                // (the whole block; scan wrote this image's counts)
  const size_t at = (size_t)n * C, rat = (size_t)n * (C / 4 + 1);
  const int M = label_compact<NTB>(E, wcount, [&](int i) { return head[at + i].x == i; },
                                   [&](int i, int rank) {
                                     if (rank < 0 || rank > C / 4) return;      // (rank <= C / 4 always: a ring has at least four cracks)
                                     ring_of[at + i] = rank;
                                     ring_head[rat + rank] = i;
                                     ring_nv[rat + rank] = place[at + i].x;      // the vertices from the head to the ring's end: all of them
                                   });
  const int T = label_scan<NTB>(ring_nv + rat, min(M, C / 4 + 1), ring_off + rat, wcount);
  for (int r = threadIdx.x; r < min(M, R); r += NTB) {
    const int e = crack[at + ring_head[rat + r]];
    long long* row = rings + ((size_t)n * R + r) * NFIELDS;           // (a2, row[4]: count cleared it, emit sums it)
    row[0] = labels[(size_t)n * HW + (e >> 2)]; row[1] = e; row[2] = ring_off[rat + r]; row[3] = ring_nv[rat + r];
  }
  if (threadIdx.x == 0) { c[1] = M; c[2] = T; c[4] = min(M, R); c[5] = min(T, V); }
}

// grid (crack blocks, images)
__global__ __launch_bounds__(NT) void ct_emit_kernel(int W, const int* __restrict__ crack, const unsigned char* __restrict__ vert, const int2* __restrict__ head,
                                                     const int2* __restrict__ place, const int* __restrict__ ring_of, const int* __restrict__ ring_off,
                                                     const int* __restrict__ counts, int C, int R, int V, long long* __restrict__ rings, int* __restrict__ xy) {
  const int n = blockIdx.y, i = blockIdx.x * NT + threadIdx.x, lane = threadIdx.x & 63;
  const int E = counts[(size_t)n * NCOUNTS + TAKEN];
  if ((int)(blockIdx.x * NT) >= E) return;                           // (the whole block)
  const size_t at = (size_t)n * C, rat = (size_t)n * (C / 4 + 1);
  int r = -1;
  long long term = 0;
  if (i < E) {
    const int e = crack[at + i], s = e & 3, p = e >> 2, y = p / W, x = p - y * W;
    const int x0 = x + (int)(s == 1 || s == 2), y0 = y + (int)(s >= 2), x1 = x0 + side_dx(s), y1 = y0 + side_dy(s);
    term = (long long)x0 * y1 - (long long)x1 * y0;
    const int h = head[at + i].x;
    r = ring_of[at + h];
    if ((unsigned)r >= (unsigned)counts[(size_t)n * NCOUNTS + 1]) r = -1;      // (never: h is a head, and rank gave it a ring below M)
    else if (vert[at + i]) {
      const int t = ring_off[rat + r] + place[at + h].x - place[at + i].x;
      if ((unsigned)t < (unsigned)V) reinterpret_cast<int2*>(xy)[(size_t)n * V + t] = make_int2(x0, y0);
    }
  }
  // a2: neighbours in compact order mostly share a ring, so the terms are summed over the runs of equal ring in the wave (MI355X
  // guide, Guideline 12: reduce before the atomic) and a run's last lane adds the sum
  const int before = __shfl_up(r, 1, 64);
  const bool starts = lane == 0 || r != before;
  const unsigned long long runs = __ballot(starts);
  const long long inc = wave_scan_ll(term);
  const int start = 63 - __clzll((long long)(runs & (~0ull >> (63 - lane))));      // the lane my run starts at
  const long long below = __shfl(inc, max(start - 1, 0), 64);
  const bool last = lane == 63 || ((runs >> (lane + 1)) & 1ull);
  if (last && r >= 0 && r < R)
    atomicAdd(reinterpret_cast<unsigned long long*>(rings + ((size_t)n * R + r) * NFIELDS + 4), (unsigned long long)(inc - (start > 0 ? below : 0)));
}

}  // namespace

ContourWs contour_carve(int N, int H, int W, int C, void* base) {
  ContourWs w{};
  camo_abi::Carver c(base);
  const size_t HW = (size_t)H * W, chunks = (HW + NT - 1) / NT, cracks = (size_t)N * C, ring_rows = (size_t)N * (C / 4 + 1);
  const bool lds = C <= CT_LDS_CRACKS;
  w.pix = c.take<unsigned short>((size_t)N * HW);
  w.cnt = c.take<int>((size_t)N * chunks);
  w.pre = c.take<int>((size_t)N * chunks);
  w.next = c.take<int>(cracks);
  w.crack = c.take<int>(cracks);
  w.vert = c.take<unsigned char>(cracks);
  w.pair[0] = c.take<int2>(cracks);
  w.pair[1] = c.take<int2>(cracks);
  w.pair[2] = lds ? nullptr : c.take<int2>(cracks);
  w.ring_of = c.take<int>(cracks);
  w.ring_head = c.take<int>(ring_rows);
  w.ring_nv = c.take<int>(ring_rows);
  w.ring_off = c.take<int>(ring_rows);
  for (w.rounds = 0; (1ll << w.rounds) < C; ++w.rounds) {}
  // global form: head round k writes pair[k & 1]; the place rounds alternate between the other of the two and pair[2]
  w.head_at = lds ? 0 : (w.rounds - 1) & 1;
  w.place_at = lds ? 1 : ((w.rounds - 1) & 1) ? 2 : 1 - w.head_at;
  w.bytes = c.bytes();
  return w;
}

int launch_contours(const int* labels, int N, int H, int W, int connectivity, int C, int R, int V, const ContourWs& ws, long long* rings, int* xy,
                    int* counts, hipStream_t stream) {
  const int chunks = (int)(((long long)H * W + NT - 1) / NT);
  const dim3 pixels((unsigned)chunks, (unsigned)N), cracks((unsigned)((C + NT - 1) / NT), (unsigned)N);
  hipLaunchKernelGGL(ct_count_kernel, pixels, dim3(NT), 0, stream, labels, H, W, chunks, R, V, ws.pix, ws.cnt, rings, xy);
  hipLaunchKernelGGL(ct_scan_kernel, dim3(N), dim3(NTB), 0, stream, ws.cnt, chunks, C, ws.pre, counts);
  if (C < 4) return (int)hipGetLastError();                          // no ring fits: scan's counts are final
  hipLaunchKernelGGL(ct_link_kernel, pixels, dim3(NT), 0, stream, labels, H, W, chunks, (int)(connectivity == 8), C, ws.pix, ws.pre, counts, ws.next, ws.crack,
                     ws.vert);
  if (C <= CT_LDS_CRACKS) {
    launch_lds<ct_doubling_kernel>(dim3(N), dim3(NTB), LDS_BYTES, stream, ws.next, ws.vert, counts, C, ws.pair[0], ws.pair[1]);
  } else {
    for (int k = 0; k < ws.rounds; ++k) {
      if (k == 0) hipLaunchKernelGGL(ct_head_round_kernel<true>, cracks, dim3(NT), 0, stream, ws.next, static_cast<const int2*>(nullptr), ws.pair[0], counts, C);
      else hipLaunchKernelGGL(ct_head_round_kernel<false>, cracks, dim3(NT), 0, stream, ws.next, ws.pair[(k - 1) & 1], ws.pair[k & 1], counts, C);
    }
    int2* const two[2] = {ws.pair[1 - ws.head_at], ws.pair[2]};
    for (int k = 0; k < ws.rounds; ++k) {
      if (k == 0) hipLaunchKernelGGL(ct_place_round_kernel<true>, cracks, dim3(NT), 0, stream, ws.next, ws.vert, ws.pair[ws.head_at], static_cast<const int2*>(nullptr), two[0], counts, C);
      else hipLaunchKernelGGL(ct_place_round_kernel<false>, cracks, dim3(NT), 0, stream, ws.next, ws.vert, ws.pair[ws.head_at], two[(k - 1) & 1], two[k & 1], counts, C);
    }
  }
  hipLaunchKernelGGL(ct_rank_kernel, dim3(N), dim3(NTB), 0, stream, labels, H * W, ws.crack, ws.pair[ws.head_at], ws.pair[ws.place_at], C, R, V, ws.ring_of,
                     ws.ring_head, ws.ring_nv, ws.ring_off, rings, counts);
  hipLaunchKernelGGL(ct_emit_kernel, cracks, dim3(NT), 0, stream, W, ws.crack, ws.vert, ws.pair[ws.head_at], ws.pair[ws.place_at], ws.ring_of, ws.ring_off,
                     counts, C, R, V, rings, xy);
  return (int)hipGetLastError();
}
