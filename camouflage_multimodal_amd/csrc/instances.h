// Object instances of a predicted mask (instances.hip, include/camo_instances.h): the constants the kernels, the
// launcher and the entry points share.  The launcher returns hipError_t as int.
#pragma once
#include "common.h"

constexpr int INST_TILE = 32;      // a labelling block's tile is INST_TILE x INST_TILE pixels of one image
constexpr int INST_NT = 256;       // threads per block of every kernel here
constexpr int INST_CHUNK = 1024;   // consecutive pixels of one image a block of the raster kernels takes (4 per thread)

struct InstWs {
  int* bgpar;              // [N][H][W] union-find parent of the background pass (fill_holes), -1 on foreground; afterwards
                           //           rid[root] = the id of the root's component, 0 when it was dropped (the same memory)
  int* par;                // [N][H][W] union-find parent of the foreground pass (index into the whole batch), -1 on background
  int* area;               // [N][H][W] area[root] = pixels of the root's component
  unsigned char* border;   // [N][H][W] border[root] = the root's background component touches the image's border
  int* chunk;              // [3][N][chunks] per chunk: kept roots (then their exclusive prefix), dropped roots, pixels of the kept
  int* misc;               // [N] holes filled
  size_t bytes;
};
InstWs inst_carve(int N, int H, int W, void* base);

int launch_instances(const float* pred, long long stride, float threshold, int N, int H, int W, int connectivity, int min_area, bool fill_holes,
                     int max_instances, const InstWs& ws, int* labels, unsigned char* clean, long long* table, int* counts, hipStream_t stream);
