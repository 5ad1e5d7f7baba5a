// Region-graph construction downstream of the superpixel segmentation: the body of the reference's create_region_graph
// (models/region_graph/extract_rg_embeddings.py:154-236) between its skimage calls, as segmented reductions over the
// label map.  Memory-bound integer / byte work on a 256 x 256 image (0.9 MB in, < 0.2 MB out): five small launches.
//
//   clear      zero the accumulators and the adjacency matrix
//   accumulate one thread per pixel p with label r:
//                own sums into acc[r] (f64 atomics: the reference's arithmetic is float64 and the variances are
//                differences of nearly equal sums): count, RGB, RGB^2, luma, luma^2, y, x, edge-map
//                perimeter[l] += 1 for every distinct label l != r among p's 4-neighbours      (|dilate(mask_l) xor mask_l| [:184])
//                ring sums of l (RGB, count) += p for every distinct l != r within L1 distance 2 (dilate(mask_l, iterations=2) & ~mask_l [:191-192])
//                adj[min][max] = 1 for every 8-neighbour label != r                              (RAG, connectivity 2 [:215])
//   finalize   one block: compaction of the non-empty labels (region_id_map [:231]), 15 features per kept region [:201-212]
//   count      one block per label a: kept neighbours b > a
//   emit       scan of the counts (one block), then per label a its pairs (i, j), (j, i) with the weight [:226-234]
#include <hip/hip_runtime.h>
#include "abi_util.h"
#include "label_inl.h"
#include "rg_features.h"

namespace {

enum { A_CNT = 0, A_R, A_G, A_B, A_RR, A_GG, A_BB, A_L, A_LL, A_Y, A_X, A_E, A_PERIM, A_NR, A_NG, A_NB, A_NCNT, A_PAD };
static_assert(A_PAD + 1 == RGF_NACC, "accumulator layout");

__global__ void rgf_clear_kernel(double* acc, size_t nacc, unsigned int* adj_words, size_t nwords) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = i; k < nacc; k += stride) acc[k] = 0.0;
  for (size_t k = i; k < nwords; k += stride) adj_words[k] = 0u;
}

__global__ __launch_bounds__(256) void rgf_accumulate_kernel(const float* __restrict__ image, const int* __restrict__ seg,
                                                             const unsigned char* __restrict__ canny, int H, int W, int n_labels,
                                                             double* __restrict__ acc, unsigned char* __restrict__ adj) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int y = p / W, x = p - y * W;
  const int r = seg[p];
  if (r < 0 || r >= n_labels) return;                          // (the host wrapper validates the label range)
  const double cr = image[3 * (size_t)p], cg = image[3 * (size_t)p + 1], cb = image[3 * (size_t)p + 2];
  const double luma = cr * 0.2989 + cg * 0.5870 + cb * 0.1140;  // np.dot(image, [0.2989, 0.5870, 0.1140]) [:151]
  double* a = acc + (size_t)r * RGF_NACC;
  atomicAdd(a + A_CNT, 1.0);
  atomicAdd(a + A_R, cr); atomicAdd(a + A_G, cg); atomicAdd(a + A_B, cb);
  atomicAdd(a + A_RR, cr * cr); atomicAdd(a + A_GG, cg * cg); atomicAdd(a + A_BB, cb * cb);
  atomicAdd(a + A_L, luma); atomicAdd(a + A_LL, luma * luma);
  atomicAdd(a + A_Y, (double)y); atomicAdd(a + A_X, (double)x);
  if (canny[p]) atomicAdd(a + A_E, 1.0);
  rg_visit_neighbours(
      r,
      [&](int ddy, int ddx) {
        const int yy = y + ddy, xx = x + ddx;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return -1;
        const int l = seg[yy * W + xx];
        return l < n_labels ? l : -1;
      },
      [&](int l) { adj[(size_t)min(l, r) * n_labels + max(l, r)] = 1; },      // (every writer stores the same byte)
      [&](int l, bool four) {
        double* b = acc + (size_t)l * RGF_NACC;
        if (four) atomicAdd(b + A_PERIM, 1.0);
        atomicAdd(b + A_NR, cr); atomicAdd(b + A_NG, cg); atomicAdd(b + A_NB, cb); atomicAdd(b + A_NCNT, 1.0);
      });
}

// one block of 1024 threads; n_labels <= 4096
__global__ __launch_bounds__(1024) void rgf_finalize_kernel(const double* __restrict__ acc, int n_labels, float* __restrict__ x,
                                                            int* __restrict__ region_map, int* __restrict__ counts) {
  __shared__ int wsum[16];
  const int kept = label_compact<1024>(
      n_labels, wsum, [&](int r) { return acc[(size_t)r * RGF_NACC + A_CNT] > 0.0; },
      [&](int r, int rank) {
        region_map[r] = rank;
        if (rank < 0) return;
        const double* a = acc + (size_t)r * RGF_NACC;
        const double n = a[A_CNT], inv = 1.0 / n;
        const double mr = a[A_R] * inv, mg = a[A_G] * inv, mb = a[A_B] * inv, ml = a[A_L] * inv;
        double contrast = 0.0;
        if (a[A_NCNT] > 0.0) {
          const double q = 1.0 / a[A_NCNT];
          const double d0 = mr - a[A_NR] * q, d1 = mg - a[A_NG] * q, d2 = mb - a[A_NB] * q;
          contrast = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        }
        // (how the compiler contracts these four differences is part of the result)
        rg_store_features(x + (size_t)rank * RGF_NFEAT,
                          {mr, mg, mb, ml, fmax(a[A_RR] * inv - mr * mr, 0.0), fmax(a[A_GG] * inv - mg * mg, 0.0),
                           fmax(a[A_BB] * inv - mb * mb, 0.0), fmax(a[A_LL] * inv - ml * ml, 0.0), a[A_X] * inv, a[A_Y] * inv, n,
                           a[A_PERIM], contrast, a[A_E] * inv});
      });
  if (threadIdx.x == 0) counts[0] = kept;
}

__global__ __launch_bounds__(256) void rgf_count_kernel(const unsigned char* __restrict__ adj, const int* __restrict__ region_map, int n_labels,
                                                        int* __restrict__ rowcount) {
  __shared__ int red[4];
  const int a = blockIdx.x, tid = threadIdx.x;
  int c = 0;
  if (region_map[a] >= 0)
    for (int b = a + 1 + tid; b < n_labels; b += 256) c += (adj[(size_t)a * n_labels + b] && region_map[b] >= 0) ? 1 : 0;
  c = wave_sum_int(c);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) rowcount[a] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(1024) void rgf_scan_kernel(const int* __restrict__ rowcount, int n_labels, int* __restrict__ rowoff, int* __restrict__ counts) {
  __shared__ int wsum[16];
  const int pairs = label_scan<1024>(rowcount, n_labels, rowoff, wsum);
  if (threadIdx.x == 0) { rowoff[n_labels] = pairs; counts[1] = 2 * pairs; }
}

// one wave per label a: its kept neighbours b > a in increasing order
__global__ __launch_bounds__(64) void rgf_emit_kernel(const unsigned char* __restrict__ adj, const int* __restrict__ region_map, const int* __restrict__ rowoff,
                                                      const float* __restrict__ x, int n_labels, long long* __restrict__ edge_index,
                                                      float* __restrict__ edge_attr, int edge_capacity) {
  const int a = blockIdx.x;
  const int i = region_map[a];
  if (i < 0) return;
  rg_emit_row(
      a, n_labels, rowoff[a], i, x, [&](int b) { return adj[(size_t)a * n_labels + b] && region_map[b] >= 0; },
      [&](int b) { return region_map[b]; }, edge_index, edge_attr, edge_capacity);
}

}  // namespace

RgGraphWs rg_graph_carve(int n_labels, void* base) {
  RgGraphWs w{};
  camo_abi::Carver c(base);
  w.acc = c.take<double>((size_t)n_labels * RGF_NACC);
  w.adj = c.take<unsigned char>(((size_t)n_labels * n_labels + 3) & ~(size_t)3);
  w.rowcount = c.take<int>((size_t)n_labels);
  w.rowoff = c.take<int>((size_t)n_labels + 1);
  w.bytes = c.bytes();
  return w;
}

int launch_region_graph(const float* image, const int* segments, const unsigned char* canny, int H, int W, int n_labels,
                        const RgGraphWs& ws, float* x, int* region_map, long long* edge_index, float* edge_attr, int edge_capacity,
                        int* counts, hipStream_t stream) {
  const size_t nacc = (size_t)n_labels * RGF_NACC, nwords = ((size_t)n_labels * n_labels + 3) / 4;
  hipLaunchKernelGGL(rgf_clear_kernel, dim3(256), dim3(256), 0, stream, ws.acc, nacc, reinterpret_cast<unsigned int*>(ws.adj), nwords);
  hipLaunchKernelGGL(rgf_accumulate_kernel, dim3((H * W + 255) / 256), dim3(256), 0, stream, image, segments, canny, H, W, n_labels, ws.acc, ws.adj);
  hipLaunchKernelGGL(rgf_finalize_kernel, dim3(1), dim3(1024), 0, stream, ws.acc, n_labels, x, region_map, counts);
  hipLaunchKernelGGL(rgf_count_kernel, dim3(n_labels), dim3(256), 0, stream, ws.adj, region_map, n_labels, ws.rowcount);
  hipLaunchKernelGGL(rgf_scan_kernel, dim3(1), dim3(1024), 0, stream, ws.rowcount, n_labels, ws.rowoff, counts);
  hipLaunchKernelGGL(rgf_emit_kernel, dim3(n_labels), dim3(64), 0, stream, ws.adj, region_map, ws.rowoff, x, n_labels, edge_index, edge_attr, edge_capacity);
  return (int)hipGetLastError();
}
