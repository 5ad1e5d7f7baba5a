// Instance contours (contours.hip, include/camo_contours.h): what the kernels, the launcher and the entry point share.
// The launcher returns hipError_t as int.
#pragma once
#include "common.h"

constexpr int CT_CHUNK = 256;            // consecutive pixels (row-major) of one block of the pixel passes
constexpr int CT_LDS_CRACKS = 1 << 14;   // CAMO_CONTOUR_LDS_CRACKS: the link state of that many cracks, in two buffers, is 128 KiB of LDS

struct ContourWs {
  unsigned short* pix;     // [N][H W] per pixel: (its cracks' offset within the chunk) << 4 | the 4-bit crack mask
  int* cnt;                // [N][chunks] cracks of every chunk
  int* pre;                // the same shape: cnt's exclusive prefix within the image
  int* next;               // [N][C] a crack's successor, as a compact position
  int* crack;              // [N][C] a crack's index e = 4 (y W + x) + s
  unsigned char* vert;     // [N][C] 1: the crack starts at a vertex
  int2* pair[3];           // [N][C] (value, next) of the doublings; pair[2] only in the global form.  heads end in pair[head_at], places in pair[place_at]
  int* ring_of;            // [N][C] at a head's position: its ring's rank
  int* ring_head;          // [N][C / 4 + 1] a ring's head position
  int* ring_nv;            // the same shape: its vertex count
  int* ring_off;           // the same shape: the offset of its first vertex
  int rounds, head_at, place_at;      // K = ceil(log2 C); where the finished doublings lie
  size_t bytes;
};
ContourWs contour_carve(int N, int H, int W, int C, void* base);

int launch_contours(const int* labels, int N, int H, int W, int connectivity, int C, int R, int V, const ContourWs& ws, long long* rings, int* xy,
                    int* counts, hipStream_t stream);
