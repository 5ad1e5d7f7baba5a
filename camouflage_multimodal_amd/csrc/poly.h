// COCO polygon annotations (poly.hip, include/camo_poly.h): what the kernels, the launcher and the entry points share.
// The launcher returns hipError_t as int.
#pragma once
#include "common.h"

struct PolyWs {
  unsigned* plane;         // [P][stride] one bit per position p = x H + y of every polygon: the toggles, then (after the scan) the mask
  int* poly_ok;            // [P] step 7 of the header for one polygon: at least one vertex, every coordinate finite and inside the margin
  int* ann_ok;             // [A] the verdict of the annotation: image and value in range, every polygon ok
  size_t stride;           // words of a plane: ceil(H W / 32) rounded up to 4, so every plane starts on 16 bytes
  size_t bytes;
};
PolyWs poly_carve(int H, int W, int A, int P, void* base);

int launch_poly_decode(const double* xy, int V, const int* poly_off, int P, const int* ann_poly_off, const int* ann_image, const int* ann_value,
                       int A, int N, int H, int W, const PolyWs& ws, int* labels, long long* ann_area, hipStream_t stream);
