// Camouflaged-object benchmark measures (seg_measures.hip, include/camo_seg_measures.h): the constants the kernels, the
// launchers and the tests share.
#pragma once
#include "common.h"

constexpr int SEGM_NT = 256;               // threads per block of every kernel here
constexpr int SEGM_SPAN = 16;              // consecutive pixels a lane of the fill kernel takes at a time (four 16-byte loads of pred)
constexpr int SEGM_SPANS_PER_LANE = 1;     // spans a lane takes while the grid is below SEGM_MAX_BLOCKS: 4096 pixels per block (measured at
                                           // N = 16, 352 x 352: 18.3 us per call against 28.2 us with 4 spans, the call being launch- and latency-bound)
constexpr int SEGM_MAX_BLOCKS = 256;       // blocks per image, at most
constexpr int SEGM_UNIFORM_LANES = 8;      // lanes that flush the same bin together before their counts are summed in registers
constexpr int SEGM_WF_TILE_X = 32;         // tile of the weighting kernel: 32 x 8 pixels, a halo of 3 around it
constexpr int SEGM_WF_TILE_Y = 8;
