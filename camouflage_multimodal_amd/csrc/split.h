// Instance splitter (split.hip, split_geo.hip, split_merge.hip, split_inl.h; include/camo_split.h, include/camo_split_geo.h,
// include/camo_split_merge.h): the
// constants the kernels, the launchers and the entry points share.  The launchers return hipError_t as int.
#pragma once
#include "common.h"

constexpr int SPLIT_IDS = 1025;        // an image's per-id arrays: entry 0 (background) and CAMO_IM_MAX_IDS ids
constexpr int SPLIT_IDS_PAD = 1088;    // ints between two images' per-id arrays
constexpr int SPLIT_MAX_SLOTS = 8;     // CAMO_SPLIT_MAX_SPLIT
constexpr int SPLIT_MAX_SIDE = 2048;   // CAMO_SEG_WF_MAX_SIDE: a row of column distances in LDS

struct SplitWs {
  int* d2;                 // [N][H][W] the nearest background row of the pixel's column, then D2 (-1: the image has no background)
  int* par;                // [N][H][W] union-find parent of the core pixels (index into the whole batch), -1 elsewhere
  int* area;               // [N][H][W] area[root] = pixels of the root's core
  int* rid;                // [N][H][W] rid[root] = the new id of a kept core of a split id
  short* site;             // [N][max_split][H][W] the nearest site row of the slot's id in the pixel's column, -1: none (null for the
                           // geodesic call, which has no sites)
  int* chunk;              // [N][max_split][chunks] per chunk the slot's kept cores, then their exclusive prefix
  int* m2;                 // [N][SPLIT_IDS_PAD] M2(id) + 2, 0: the id has no pixel
  int* ncore;              // [N][SPLIT_IDS_PAD] the id's kept cores
  int* parts;              // [N][SPLIT_IDS_PAD] the id's parts
  int* first;              // [N][SPLIT_IDS_PAD] the parts of the ids before it: its first new id - 1
  int* slot_of;            // [N][SPLIT_IDS_PAD] the id's split slot, -1: it stays whole
  int* slot_id;            // [N][SPLIT_MAX_SLOTS] the slot's id, 0: free
  int* dropped;            // [N] cores dropped as small
  size_t bytes;
};
SplitWs split_carve(int N, int H, int W, int max_split, void* base, bool sites = true);

int launch_split(const int* labels, const float* pred, long long stride, int N, int H, int W, int num, int den, int min_core, int max_split,
                 int max_instances, const SplitWs& ws, int* out, long long* table, int* counts, hipStream_t stream);

// ---- low-dynamic cores merged (split_merge.hip, include/camo_split_merge.h) -------------------------------------------
struct SplitMergeWs {
  int* d2;                   // [N][H][W] the nearest background row of the pixel's column, then D2 (-1: the image has no background)
  unsigned long long* pass;  // [N][SPLIT_IDS_PAD] per part (its best contact value with a higher part << 11) | (2047 - that part), 0: none
  int* peak;                 // [N][SPLIT_IDS_PAD] peak(part) + 2, 0: the part has no pixel
  int* owner;                // [N][SPLIT_IDS_PAD] the largest input id over the part's pixels
  int* new_id;               // [N][SPLIT_IDS_PAD] the part's new id, 0: the part has no pixel
  int* bad;                  // [N] 1: a foreground pixel holds a part value out of range, the image is not supported
  size_t bytes;
};
SplitMergeWs split_merge_carve(int N, int H, int W, void* base);

int launch_split_merge(const int* labels, const int* parts, const float* pred, long long stride, int N, int H, int W, int num, int den,
                       int max_instances, const SplitMergeWs& ws, int* out, long long* table, int* counts, hipStream_t stream);

// ---- geodesic growth (split_geo.hip, include/camo_split_geo.h) ----------------------------------------------------
constexpr int SPLIT_GEO_TILE = 32;         // CAMO_SPLIT_GEO_TILE: a grow block's tile, INST_TILE
constexpr int SPLIT_GEO_SWEEPS = 128;      // Jacobi sweeps of one tile in one launch: 4 tile sides.  A tile still changing then flags itself

struct SplitGeoWs {
  SplitWs s;                 // the common launches' arrays, site null
  unsigned long long* key;   // [N][H][W] 0 off the split ids, else (g << 32) | (new id << 4) | (slot + 1); g = SPLIT_GEO_FAR + ...: not reached
  int* flag[2];              // [N][tiles] each: the tiles to grow in the rounds of even / odd number
  size_t bytes;
};
SplitGeoWs split_geo_carve(int N, int H, int W, int max_split, void* base);

// init, `rounds` grow launches, finish, table after the ten common launches; the resume: the grow launches, finish, table
int launch_split_geo(const int* labels, const float* pred, long long stride, int N, int H, int W, int num, int den, int min_core, int max_split,
                     int max_instances, int rounds, const SplitGeoWs& ws, int* out, long long* table, int* counts, int* pending, hipStream_t stream);
int launch_split_geo_resume(const int* labels, const float* pred, long long stride, int N, int H, int W, int max_instances, int rounds,
                            const SplitGeoWs& ws, int* out, long long* table, const int* counts, int* pending, hipStream_t stream);
