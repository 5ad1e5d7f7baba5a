// Head-averaged attention maps of the fused row-tile schedule (attn_maps.hip): one launch behind the forward's back half.
// The fused kernels never store probabilities, so an inference call that wants the two maps recomputes them here from the
// tensors the front half left in the workspace (bf16 queries / keys of both directions) and the KG->RG softmax statistics the
// back half's combine step stored.  Returns hipError_t as int.
#pragma once
#include "fused_rows.h"

struct AttnMapsArgs {
  const us16* Q16; const us16* KV16;           // RG queries (pre-scaled) [T][256]; KG keys|values [B*Nk][512]
  const us16* Q2_16; const us16* KV2_16;       // KG queries (pre-scaled) [B*Nk][256]; RG keys|values [T][512]
  const float* lse2;                           // [B][8][16][2]: {max, sum} of the KG->RG softmax per (sample, head, query)
  const int4* tile_desc;                       // the batch descriptor's table: per 32-row RG tile {sample, first packed row, rows, -}; sample = -1 past the last tile
  float* rg2kg; float* kg2rg;                  // out [T][Nk] each (either may be null): row t = RG node t; kg2rg element (t, j) = weight of KG query j on RG key t
  int Nk, tiles, rows_rg;                      // tiles = entries of tile_desc (grid size); rows_rg = T (launch-timing bookkeeping only)
};
int launch_attn_maps(const AttnMapsArgs& a, hipStream_t stream);
