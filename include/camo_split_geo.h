/* C ABI of geodesic growth for the instance splitter on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * camo_split_instances (include/camo_split.h) gives every pixel of a split id to the core with the Euclidean-nearest core pixel, so a
 * part is a Voronoi cell cut to the id and, in a concave id -- a coiled snake, an arm curled round another animal --, comes out in
 * several pieces: a stretch of one animal goes to the other across a background gap.  camo_split_instances_geodesic measures the
 * distance INSIDE the id instead, along 8-neighbour paths at the 5-7 chamfer weights, so every part is one 8-connected piece that
 * contains its core.  Only integers are compared and added and every tie has a rule, so where the call reports an image as finished
 * every output byte of that image is a function of the inputs alone.
 * PARITY UNPINNED, as in camo_split.h: the text below is the definition; it is restated sequentially in numpy, with a heap Dijkstra,
 * in tests/split_geo_ref.py, which the kernels are tested against byte for byte.
 *
 * Steps 1 - 3 and 5 - 8 of camo_split_instances hold unchanged: D2, the cores, the kept cores, the qualifying and the split ids, the
 * numbering of the parts, out_labels, the table and counts.  Step 4 is replaced by
 *   4g. The pixels of one split id are a graph: two of them are linked when they are 8-neighbours.  A horizontal or vertical link
 *       costs 5 and a diagonal link 7; a diagonal link exists whenever both its ends have the id, whatever the two pixels beside it
 *       hold.  g(p, c) = the cheapest path cost from the pixel p to any pixel of the kept core c of the same id, 0 on the core
 *       itself.  p goes to the kept core of smallest (g(p, c), new id of c) in lexicographic order: equal costs go to the core that
 *       comes first in reading order, because step 5 numbers an id's parts in the row-major order of their cores' first pixels.  The
 *       pixels of dropped cores are ordinary pixels.  A pixel of a split id that no kept core reaches -- the caller's id is not
 *       8-connected -- goes to the id's first part, the one with the smallest new id.  The pixels of another id are never crossed and
 *       never candidates.
 * Every part is 8-connected and contains its core: every pixel of a cheapest path takes the core its end takes.
 *
 * The key (g, new id) of a pixel is the smallest of its own start -- (0, new id) on a kept core pixel -- and (g_q + w, id_q) over
 * its linked neighbours q.  Adding the same w keeps the lexicographic order and w > 0, so these equations have ONE solution, and
 * relaxing them in any order reaches it.  The growth runs in ROUNDS: a round is one launch with one block per 32 x 32 tile; a tile
 * does work only when a neighbour's edge (or its own cores) changed in the round before.  `rounds` is the number of rounds the call
 * enqueues -- the launches are a function of rounds alone, and the library never synchronises --, and pending[n] tells how many tiles
 * of image n still had work:
 *   counts is final after the call, whatever rounds is: it does not depend on growth.
 *   Where pending[n] == 0, image n's out_labels and table rows are final: the bytes of the definition above.
 *   Where pending[n] != 0, they are valid (every foreground pixel holds a new id of its own input id, the table is that of
 *   out_labels) but unspecified: they depend on which of its neighbours' keys a block happened to read.
 * camo_split_geodesic_resume enqueues `rounds` more on the workspace such a call left, so a caller reaches the definition for any
 * content by reading pending between calls.  tiles_x + tiles_y rounds are enough for every path that is monotone in both axes, a
 * convex blob among them; a corridor needs about one round per tile border it crosses, and one more per CAMO_SPLIT_GEO_TILE * 4
 * pixels it runs inside one tile.
 * Marker merging is a post-pass on the parts of either growth: include/camo_split_merge.h.
 * Not built here either: a per-component absolute radius.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_SPLIT_GEO_H
#define CAMO_SPLIT_GEO_H
#include <stddef.h>
#include <stdint.h>
#include "camo_split.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_SPLIT_GEO_TILE 32            /* side of a tile: tiles_x = ceil(W / 32), tiles_y = ceil(H / 32) */
#define CAMO_SPLIT_GEO_MAX_ROUNDS 1024    /* rounds of one call: what bounds the launches one call enqueues */
#define CAMO_SPLIT_GEO_LAUNCHES 13        /* kernel launches of camo_split_instances_geodesic besides its `rounds` grow launches */
#define CAMO_SPLIT_GEO_RESUME_LAUNCHES 2  /* kernel launches of camo_split_geodesic_resume besides its `rounds` grow launches */

/* Bytes of the workspace of the two calls below (camo_split_workspace_bytes without its site planes, plus a 64-bit key per pixel and
 * two flags per tile); 0 when the arguments are not supported (the limits of camo_split_workspace_bytes). */
size_t camo_split_geodesic_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t max_split);

/* camo_split_instances with step 4g, in CAMO_SPLIT_GEO_LAUNCHES + rounds launches.  Every argument up to `stream` is
 * camo_split_instances', with ws of camo_split_geodesic_workspace_bytes(N, H, W, max_split) bytes; pending int32 [N] as above.
 * Needs what camo_split_instances needs, 1 <= rounds <= CAMO_SPLIT_GEO_MAX_ROUNDS and pending not null: otherwise CAMO_E_ARG.  What
 * ws and the four outputs hold on entry is unspecified; every element of out_labels, table, counts and pending is written.
 *
 * The launches:
 *   column .. rank   the first ten launches of camo_split_instances: after them every kept core of a split id has its new id, and
 *                    the pixels that are not split are written
 *   init             per pixel a 64-bit key (g << 32 | new id << 4 | split slot + 1): g = 0 with the core's new id on the kept core
 *                    pixels of the split ids, a cost above every path's (2^30; g < 7 * 2048^2 < 2^25) on their other pixels, 0 off
 *                    the split ids.  A tile is flagged for round 0 when it, or the one-pixel ring around it, holds such a core pixel;
 *                    the flags are double-buffered by the round's parity
 *   grow (rounds)    one block per tile.  A block whose flag of this round is clear returns at once.  Otherwise it loads its 34 x 34
 *                    keys, the ring around the tile included, into LDS (9.5 KB) and relaxes them there by Jacobi sweeps to the tile's
 *                    own fixed point, at most 4 * CAMO_SPLIT_GEO_TILE sweeps; it stores the keys of its tile that went down with
 *                    plain 64-bit stores, and where a pixel of the tile's outer ring went down it sets the next round's flag of the
 *                    tiles that touch that pixel -- and its own when the last sweep still changed a key
 *   finish           out_labels from the keys, with the first-part rule where g is still above every path's; the table cleared;
 *                    pending[n] = the tiles of image n flagged for the round that was not run
 *   table            as in camo_split_instances
 * No block waits for another: no spin, no grid barrier, no cooperative launch; every loop in a kernel is bounded by the tile size.
 * Integer atomics only: those of camo_split_instances; the growth itself uses none on memory. */
int camo_split_instances_geodesic(const int32_t* labels, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W,
                                  int32_t ratio_num, int32_t ratio_den, int32_t min_core, int32_t max_split, int32_t max_instances,
                                  int32_t* out_labels, int64_t* table, int32_t* counts, void* ws, size_t ws_bytes, void* stream,
                                  int32_t rounds, int32_t* pending);

/* `rounds` more grow launches, then finish and table: CAMO_SPLIT_GEO_RESUME_LAUNCHES + rounds launches.  The arguments and their
 * checks are those of camo_split_instances_geodesic; labels, pred, the sizes, the settings and ws must be the ones of the geodesic
 * call (or resume) before it, with ws and counts as that call left them -- counts is read, not written.  Every element of out_labels,
 * table and pending is written, under the contract above. */
int camo_split_geodesic_resume(const int32_t* labels, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W,
                               int32_t ratio_num, int32_t ratio_den, int32_t min_core, int32_t max_split, int32_t max_instances,
                               int32_t* out_labels, int64_t* table, int32_t* counts, void* ws, size_t ws_bytes, void* stream,
                               int32_t rounds, int32_t* pending);

#ifdef __cplusplus
}
#endif
#endif
