// SLIC superpixel label maps for a batch of images (slic.hip): quantise / smooth / Lab, ten rounds of windowed nearest-centroid
// assignment and integer-summed centroid means, connectivity enforcement by union-find.  All launchers return hipError_t as int.
#pragma once
#include "canny.h"

constexpr int SLIC_TILE = 32;             // a block's tile is SLIC_TILE x SLIC_TILE pixels of one image
constexpr int SLIC_CHUNK = 1024;          // pixels of one image per block in the raster-order passes of the connectivity stage
constexpr int SLIC_ITERATIONS = 10;

struct SlicGrid { int K, step, start, ny, nx; };

struct SlicConnWs {
  int* parent;             // [N][H][W] union-find parent (index into the whole batch); the root once flattened
  int* size;               // [N][H][W] size[root] = pixels of the root's component
  int* adj;                // [N][H][W] adj[root]: small component -> root of the component it adopts the label of (-1: none);
                           //           large component -> its new label
  int* queue;              // [N][H][W] search queues of the small components, carved by a bump counter
  unsigned char* mark;     // [N][H][W] pixel already in its component's queue
  int* chunk;              // [N][chunks] large components whose first pixel lies in the chunk, then the exclusive prefix
  int* misc;               // [0] queue cursor, [1 + n] components of max_size pixels or more in image n
  size_t bytes;
};
struct SlicWs {
  SlicConnWs conn;
  float* lab;              // [N][H][W][3]
  int* nearest;            // [N][H][W]
  float* cent;             // [N][K][5]
  long long* sums;         // [N][K][6] sums of y, x, L, a, b (colours in 2^-24 units) and the pixel count
  size_t bytes;
};
SlicConnWs slic_conn_carve(int N, int H, int W, void* base);
SlicWs slic_carve(int N, int H, int W, int K, void* base);

int launch_slic_preprocess(const float* images, int N, int H, int W, const CannyTaps& taps, float inv_compactness, float* lab, hipStream_t stream);
// centroids on the grid with zero colour, sums cleared
int launch_slic_init(const SlicGrid& g, int N, float* cent, long long* sums, hipStream_t stream);
// dist may be null
int launch_slic_assign(const float* lab, const float* cent, int N, int H, int W, int K, int step, int* nearest, float* dist, hipStream_t stream);
// clear_first: the sums hold anything; otherwise they are clear (every update leaves them so)
int launch_slic_update(const float* lab, const int* nearest, int N, int H, int W, int K, long long* sums, float* cent, bool clear_first,
                       hipStream_t stream);
int launch_slic_connect(const int* labels_in, int N, int H, int W, int min_size, int max_size, const SlicConnWs& ws, int* labels, int* counts,
                        hipStream_t stream);
