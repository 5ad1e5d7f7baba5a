/* C ABI of the instance splitter on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * camo_instances (include/camo_instances.h) finds objects as connected components of the mask, so two camouflaged animals that touch,
 * or that one superpixel bridges, come out as ONE instance: one false positive and two false negatives at every IoU threshold.
 * camo_split_instances splits such a component at its necks.  The squared Euclidean distance to the background is large in the body
 * of an object and small in a neck, so the pixels whose distance is above a fraction of the component's largest distance fall into
 * one CORE per body; a component with two cores or more is divided among them, every pixel to the core with the nearest core pixel.
 * Only integers are compared and summed, a core's root is its smallest pixel index and every tie has a rule, so every output byte is a
 * function of the inputs alone (two calls give the same bytes, a batch gives the rows of its images one by one).
 * PARITY UNPINNED: the reference has no instance extraction, and scipy.ndimage / skimage.segmentation.watershed are not part of this
 * package, so their conventions are not pinned.  The text below is the definition; it is restated sequentially in numpy, with a
 * brute-force distance transform and a brute-force nearest site, in tests/split_ref.py, which the kernels are tested against byte for
 * byte.
 * A cell is a Euclidean Voronoi cell of its core cut to the component, and in a concave component it may come out in several pieces:
 * include/camo_split_geo.h grows connected cells along paths inside the component instead.
 * One level set cuts a low lobe off its body as readily as a body off its neighbour: include/camo_split_merge.h joins the parts again
 * whose pass to a higher part is nearly as high as their own peak.  Not built: a per-component absolute radius.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_SPLIT_H
#define CAMO_SPLIT_H
#include <stddef.h>
#include <stdint.h>
#include "camo_instances.h"
#include "camo_inst_match.h"
#include "camo_seg_measures.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_SPLIT_MAX_SPLIT 8      /* max_split: ids split per image */
#define CAMO_SPLIT_MAX_DEN 16       /* ratio_den */
#define CAMO_SPLIT_COUNTS 4         /* int32 per image */
#define CAMO_SPLIT_LAUNCHES 13      /* kernel launches of one call, whatever N and the content */

/* Bytes of camo_split_instances' workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_split_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t max_split);

/* Splits the touching objects of a label map in CAMO_SPLIT_LAUNCHES launches (all grids over the whole batch).
 * labels int32 [N, H, W]: 0 on background, an id in 1 .. CAMO_IM_MAX_IDS elsewhere; an id is ONE input component (what camo_instances
 * writes qualifies, at either connectivity; the pixels of an id need not be connected).  A value outside 0 .. CAMO_IM_MAX_IDS is
 * read as 0.  pred: null, or the probability plane of camo_instances -- image i's [H, W] plane starts at pred + i * pred_image_stride
 * floats (one channel of a [N, C, H, W] map is read in place); it is used for the table's Sq only.  ratio = ratio_num / ratio_den.
 * ws: workspace of camo_split_workspace_bytes(N, H, W, max_split) bytes, 256-byte aligned.  Per image:
 *   1. D2(p) of a foreground pixel p = (y, x): the smallest (y - y')^2 + (x - x')^2 over the pixels (y', x') of the image with label 0.
 *      The image's edge is not background.  An image with no label-0 pixel has no D2: it has no core pixel and nothing is split.
 *   2. M2(id) = the largest D2 over the id's pixels.  A foreground pixel is a CORE PIXEL when ratio_den^2 D2 > ratio_num^2 M2(id),
 *      compared in 64 bits.  The core pixels are labelled with 8-connectivity, two touching core pixels being linked when they have the
 *      same id: a component of that is a CORE, and belongs to one id.  A core of fewer than min_core pixels is dropped (area ==
 *      min_core is kept); the others are KEPT.
 *   3. An id QUALIFIES when it keeps at least 2 cores.  The first max_split qualifying ids, in id order, are SPLIT; later
 *      qualifying ids stay whole, and so does every other id.
 *   4. Every pixel (y, x) of a split id -- its core pixels and those of its dropped cores included -- goes to the kept core OF ITS OWN
 *      ID that holds the site (y', x') of smallest ((y - y')^2 + (x - x')^2, y', x') in lexicographic order, the sites being the
 *      pixels of the id's kept cores: the nearest core pixel, a tie to the smaller y', then to the smaller x' (the rule of
 *      camo_seg_weighted_f's nearest positive pixel).  The cores of other ids are never candidates, however near.  The pixels of one
 *      core are a PART.  A part is the core's Euclidean Voronoi cell cut to the id: in a concave component it may be disconnected.
 *   5. New ids 1 .. K' number the parts in input-id order; the parts of one split id in the row-major order of their cores' first
 *      pixels; an id that stays whole is one part when it has a pixel, and takes no number when it has none.  So a map whose ids are
 *      1 .. P with a pixel each, none of them split, comes back unchanged.
 *   6. out_labels int32 [N, H, W]: 0 where labels reads as 0, the new id elsewhere -- all K' ids, those above max_instances included.
 *   7. table int64 [N, max_instances, CAMO_INST_FIELDS]: camo_instances' row (area, x0, y0, x1, y1, Sx, Sy, Sq) of every new id
 *      k <= max_instances, over out_labels; Sq is 0 when pred is null.  Rows past K' are zero: the call writes the whole table.
 *   8. counts int32 [N, CAMO_SPLIT_COUNTS] = (K', the ids split, the cores dropped as small -- of every id --, the qualifying ids
 *      left whole).
 * Needs camo_instances' limits on N, H and W, H and W at most CAMO_SEG_WF_MAX_SIDE, 0 < ratio_num < ratio_den <= CAMO_SPLIT_MAX_DEN,
 * min_core >= 0, 1 <= max_split <= CAMO_SPLIT_MAX_SPLIT, 1 <= max_instances, N * max_instances <= CAMO_INST_MAX_ROWS, pred null or
 * pred_image_stride >= H * W, labels, out_labels, table, counts and ws not null, labels and out_labels not overlapping, table 8-byte
 * aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise CAMO_E_ARG.  What ws and the three outputs hold
 * on entry is unspecified; every element of out_labels, table and counts is written.
 *
 * The launches:
 *   column, row      the exact distance transform of camo_seg_weighted_f: per column the nearest background row, then one block per
 *                    image row with those staged in LDS (CAMO_SEG_WF_MAX_SIDE ints) searches outwards from its own column for as
 *                    long as the column offset alone stays below the best distance; M2 by integer max, through an LDS table per row
 *   tiles, join,     the cores by the tiled union-find of camo_instances with `same` = equal id (32 x 32 tiles in LDS, agent-scope
 *   flatten          atomicMin on the larger root), and every core's area
 *   cores, ids       the kept cores of every id counted; one block per image ranks the qualifying ids, names the split ones and
 *                    scans the parts of every id into the first new id of each
 *   count, scan,     per split id the kept cores of every chunk of 1024 pixels, their prefix, and so each core's rank among its
 *   rank             id's: its new id.  The rank launch also writes out_labels of everything that is not split and clears the table
 *   sites, nearest   once per (image, split slot) -- N * max_split virtual images --: per column the nearest site row of that id,
 *                    then one block per row: the id's pixels search outwards as above under the tie rule and write their core's id
 *   table            camo_instances' run records and LDS slots over out_labels
 * Integer atomics only: add, min, max (and the compare-and-swap of the LDS slots). */
int camo_split_instances(const int32_t* labels, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H, int32_t W,
                         int32_t ratio_num, int32_t ratio_den, int32_t min_core, int32_t max_split, int32_t max_instances,
                         int32_t* out_labels, int64_t* table, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
