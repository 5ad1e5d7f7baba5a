/* C ABI of marker merging for the instance splitter on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * camo_split_instances (include/camo_split.h) and camo_split_instances_geodesic (include/camo_split_geo.h) take the cores of an id
 * from ONE level set of its distance transform.  Any fixed level slices some bump between its saddle and its peak: a lobe whose peak
 * lies barely above the level, with a saddle barely below it, becomes a core of its own, and one animal is reported as two.
 * camo_split_merge suppresses such maxima of low DYNAMIC: a part is joined to a higher neighbouring part when the pass between them is
 * nearly as high as its own peak.  The criterion is local, so a real neck between two large bodies stays cut whatever the ratio is.
 * It is a post-pass on the part map: a union of Voronoi cells is the cell of the union of their sites, and the same holds for
 * geodesic cells, so relabelling the parts is growing from the merged markers, and one call serves both growths.  Only integers are
 * compared and every tie has a rule, so every output byte is a function of the inputs alone (two calls give the same bytes, a batch
 * gives the rows of its images one by one).
 * PARITY UNPINNED, as in camo_split.h: skimage.morphology.h_maxima and its kin are not part of this package, so their conventions
 * are not pinned.  The text below is the definition; it is restated sequentially in numpy, with a double loop over the neighbours
 * and plain dictionaries, in tests/split_merge_ref.py, which the kernels are tested against byte for byte.
 * Not built: reuse of the splitter's D2 (the call takes the distance transform again, two launches, so that it needs nothing from
 * a growth's workspace and runs on any part map); merging re-evaluated on the groups' peaks (the link test below is first order:
 * every part is tested once, with its own peak).
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_SPLIT_MERGE_H
#define CAMO_SPLIT_MERGE_H
#include <stddef.h>
#include <stdint.h>
#include "camo_split.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_SPLIT_MERGE_COUNTS 4       /* int32 per image */
#define CAMO_SPLIT_MERGE_LAUNCHES 6     /* kernel launches of one call, whatever N and the content */

/* Bytes of camo_split_merge's workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_split_merge_workspace_bytes(int32_t N, int32_t H, int32_t W);

/* Joins the parts of a split label map across their high passes in CAMO_SPLIT_MERGE_LAUNCHES launches (all grids over the whole batch).
 * labels int32 [N, H, W]: the splitter's input map -- 0 on background, an id in 1 .. CAMO_IM_MAX_IDS elsewhere; a value outside
 * 0 .. CAMO_IM_MAX_IDS is read as 0.  parts int32 [N, H, W]: the splitter's out_labels, or any map that holds a part id in
 * 1 .. CAMO_IM_MAX_IDS on every pixel where labels reads > 0; what it holds elsewhere is not read.  pred, pred_image_stride: as in
 * camo_split_instances, for the table's Sq only.  ratio = merge_num / merge_den.  ws: workspace of
 * camo_split_merge_workspace_bytes(N, H, W) bytes, 256-byte aligned.  Per image:
 *   1. D2(p) of a foreground pixel: exactly step 1 of camo_split_instances on labels.  An image with no label-0 pixel has no D2 and
 *      links nothing.
 *   2. peak(a) = the largest D2 over the pixels with parts == a.  The parts are ordered by (peak, the smaller part id first): b is
 *      HIGHER than a when peak(b) > peak(a), or when the peaks are equal and b < a.
 *   3. A CONTACT of a with b is a pair of 8-neighbour pixels, p in a and q in b, with a != b and the same read id in labels; a
 *      diagonal pair counts whatever the two pixels beside it hold.  Its value is min(D2(p), D2(q)).  Pixels of different ids are
 *      never a contact.
 *   4. For a part a that has a contact with a higher part, pass(a) = the largest value over its contacts with higher parts, and
 *      up(a) = the higher part that holds that value, a tie to the smaller part id.
 *   5. a is LINKED to up(a) when merge_den^2 pass(a) >= merge_num^2 peak(a), compared in 64 bits: a maximum joins across its highest
 *      pass to a higher neighbour when that pass is at least num / den of its own height, measured in distance.  Links point
 *      strictly upwards in the order, so they form a forest; a GROUP is a tree of it.  The peaks are those of the given parts: they
 *      are NOT re-evaluated after a link, and a part that is not linked itself may still be the root that others join.
 *   6. New ids 1 .. K'' number the groups in the order of each group's smallest part id; a part id without a pixel takes no number.
 *      Where nothing links, out_labels is parts with the gaps closed.
 *   7. out_labels int32 [N, H, W]: 0 where labels reads 0, the new id elsewhere -- all K'' ids, those above max_instances included.
 *   8. table int64 [N, max_instances, CAMO_INST_FIELDS]: camo_instances' row of every new id k <= max_instances, over out_labels;
 *      Sq is 0 when pred is null.  Rows past K'' are zero: the call writes the whole table.
 *   9. counts int32 [N, CAMO_SPLIT_MERGE_COUNTS] = (K'', the part ids present, the groups of two parts or more, the input ids that
 *      had two parts or more and are one part again).  A part id's OWNER is the largest read id over its pixels (the splitter's parts
 *      lie in one id each); the last count is that of the ids that own two part ids or more, all of them in one group.
 *  10. An image is NOT SUPPORTED when one of its foreground pixels holds a parts value outside 1 .. CAMO_IM_MAX_IDS: its counts are
 *      (-1, 0, 0, 0), its table rows zero, its out_labels parts where labels reads > 0 and 0 elsewhere.  No other image is affected.
 * Needs camo_split_instances' limits on N, H, W and max_instances, 0 < merge_num <= merge_den <= CAMO_SPLIT_MAX_DEN, pred null or
 * pred_image_stride >= H * W, labels, parts, out_labels, table, counts and ws not null, out_labels overlapping neither labels nor
 * parts, table 8-byte aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise CAMO_E_ARG.  What ws and the
 * three outputs hold on entry is unspecified; every element of out_labels, table and counts is written.
 *
 * The launches:
 *   column, d2   the distance transform of camo_split_instances, by the same device functions; the d2 launch leaves peak, and each
 *                part's owner, by integer max through LDS tables of CAMO_IM_MAX_IDS + 1 entries per row block, and raises the
 *                image's flag where a part value is out of range
 *   pass         chunks of 1024 pixels; a pixel looks at its E, SW, S and SE neighbours, so every unordered contact is seen once, and
 *                offers (value << 11 | 2047 - higher part) to the lower part's slot by one 64-bit atomicMax; where equal slots run
 *                together in a wave, the run's largest key is taken there and one lane issues the atomic
 *   groups       one block per image: the link test, the up pointers in LDS, 11 rounds of pointer jumping, the smallest member of
 *                every root, the ranks of those members: the new id of every part; counts
 *   relabel      out_labels; the table cleared
 *   table        camo_instances' run records and LDS slots over out_labels
 * No block waits for another; every loop in a kernel is bounded by the sizes.  Integer atomics only: add, min, max (and the
 * compare-and-swap of the LDS slots). */
int camo_split_merge(const int32_t* labels, const int32_t* parts, const float* pred, int64_t pred_image_stride, int32_t N, int32_t H,
                     int32_t W, int32_t merge_num, int32_t merge_den, int32_t max_instances, int32_t* out_labels, int64_t* table,
                     int32_t* counts, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
