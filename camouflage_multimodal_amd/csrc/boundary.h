// Boundary IoU (boundary.hip, include/camo_boundary.h): the erosion that makes the boundary maps -- what its kernels,
// its launcher and the entry point share.  The match under the combined IoU is inst_match.h's.  The launcher returns hipError_t as int.
#pragma once
#include "common.h"

constexpr int BD_NT = 256;         // threads per block of the two erosion kernels
constexpr int BD_STRIP = 64;       // rows of one image a block of the column pass takes (CAMO_BD_STRIP): one bit each in a 64-bit mask

// rowok: [N][H][W] bytes, the row pass's result
int launch_boundary_labels(const int* labels, int N, int H, int W, int d, int* out, unsigned char* rowok, hipStream_t stream);
