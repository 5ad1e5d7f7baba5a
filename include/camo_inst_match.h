/* C ABI of instance matching on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * Stands behind the question camo_instances leaves open: are the objects a predicted mask holds the right ones?  camo_inst_match
 * takes two label maps -- predicted ids and ground-truth ids, 0 = background, as camo_instances writes them -- counts the pixels of
 * every (predicted, ground-truth) pair, and matches predictions to ground truth greedily in score order at each of up to 16 IoU
 * thresholds.  Everything is integer arithmetic: IoUs are compared by cross-multiplication, thresholds are fractions, scores are the
 * exact integers of camo_instances' table, so every output byte is a function of the inputs alone (two calls give the same bytes, a
 * batch gives the rows of its images one by one).  The ratios -- IoU, precision, recall, PQ, AP -- are taken from the integers in
 * float64 on the host (camouflage_multimodal_amd/instance_match.py).
 * PARITY UNPINNED: the reference has no instance evaluation and pycocotools / panopticapi are not part of this package, so their
 * conventions are not pinned.  The text below is the definition; it is restated in numpy in tests/inst_match_ref.py, which the
 * kernels are tested against byte for byte.
 *
 * Device pointers only (thr_num excepted: a HOST array), enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok /
 * CAMO_E_ARG as in camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of
 * camo_fusion.h. */
#ifndef CAMO_INST_MATCH_H
#define CAMO_INST_MATCH_H
#include <stddef.h>
#include <stdint.h>
#include "camo_instances.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_IM_MAX_THRESHOLDS 16   /* T */
#define CAMO_IM_MAX_IDS 1024        /* P and G */
#define CAMO_IM_MAX_CELLS (1 << 26) /* N * (P + 1) * (G + 1) */
#define CAMO_IM_COUNTS 4            /* int32 per image */

/* Bytes of camo_inst_match's workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_inst_match_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t P, int32_t G, int32_t T);

/* Overlap table and greedy matches of an image batch in FOUR launches (clear, overlap, areas and ranks, match; all grids over the
 * whole batch; the count does not depend on N).  pred_labels and gt_labels are int32 [N, H, W].  P and G are the largest predicted
 * and ground-truth ids the tables hold.  pred_table is camo_instances' int64 [N, pred_table_rows, CAMO_INST_FIELDS] table, or null.
 * thr_num is a HOST array of T threshold numerators over the common denominator thr_den; it is read before the call returns.
 * ws: workspace of camo_inst_match_workspace_bytes(N, H, W, P, G, T) bytes, 256-byte aligned.  Per image:
 *   1. Overlap table.  inter int32 [N, P + 1, G + 1]: inter[p][g] is the number of pixels with predicted label p and ground-truth
 *      label g; row and column 0 are background.  A pixel with a label outside 0 .. P (predicted) or 0 .. G (ground truth) enters
 *      no cell; it is counted in counts instead.  The call writes the whole table.
 *   2. Areas.  area_p = sum over g of inter[p][g] and area_g = sum over p of inter[p][g], background column and row included: the
 *      overlap table's own sums, not a caller's table, so they agree with inter by construction.  gt_area int32 [N, G] holds
 *      area_g of ids 1 .. G.
 *   3. Score order.  Predicted id p has score Sq / area, read from fields 7 and 0 of row p - 1 of pred_table.  The row must exist
 *      (p <= pred_table_rows) and satisfy 0 < area <= CAMO_RGD_MAX_IMAGE_PIXELS and 0 <= Sq <= 255 area; otherwise the score is
 *      0 / 1.  Scores are compared exactly by 64-bit cross-multiplication (the products stay below 2^60).  Rank: score descending,
 *      ties by smaller id, over all ids 1 .. P.  With pred_table null the order is by id.
 *   4. Thresholds.  t_k = thr_num[k] / thr_den, 1 <= T <= CAMO_IM_MAX_THRESHOLDS, 1 <= thr_num[k] <= thr_den <= 1000 (the COCO
 *      set is the numerators 10 .. 19 over 20).  IoU(p, g) >= t_k is tested as thr_den i >= thr_num[k] u with i = inter[p][g] and
 *      u = area_p + area_g - i.  No float is on the path.
 *   5. Greedy match, for each k independently.  Predicted ids with area_p > 0 are taken in rank order; each takes the best
 *      still-unmatched ground-truth id that has area_g > 0, i > 0 and IoU >= t_k.  Best: highest IoU, compared by
 *      i1 u2 > i2 u1; ties go to the smaller id.  match int32 [N, T, P] holds the ground-truth id of every predicted id, or 0;
 *      gt_match int32 [N, T, G] holds the predicted id of every ground-truth id, or 0.
 *   6. Per-prediction row.  pred_rows int32 [N, P, 4] = (area_p, the 0-based rank, the ground-truth id of highest IoU over all
 *      ground-truth ids, matched or not -- 0 when it overlaps none, ties to the smaller id --, the intersection with that id).
 *   7. Counts.  counts int32 [N, CAMO_IM_COUNTS] = (pixels whose predicted label is out of range, pixels whose ground-truth label
 *      is out of range, predicted ids with area > 0, ground-truth ids with area > 0).
 * Needs camo_instances' limits on N, H and W, 1 <= P, G <= CAMO_IM_MAX_IDS, N (P + 1) (G + 1) <= CAMO_IM_MAX_CELLS, the thresholds
 * as in 4, pred_table_rows >= 1 when pred_table is given and the table 8-byte aligned, no other null pointer, ws 256-byte aligned
 * and ws_bytes at least the workspace size: otherwise CAMO_E_ARG.
 * What ws and the six outputs hold on entry is unspecified; every element of inter, pred_rows, gt_area, match, gt_match and counts
 * is written.
 *
 * The overlap launch is the only pixel-rate pass: a block takes 1024 consecutive pixels of one image, a run of consecutive lanes
 * with the same pair is one record (its length), a record goes to the pair's slot of a small LDS table (to memory when every slot
 * holds another pair) and the block adds its slots to inter once.  The match launch is one block per (threshold, image) with the
 * rank order, the areas and the matched flags in LDS, and up to 16 more blocks per image for 6 and the last two of 7.  32-bit INTEGER atomic adds only: no floating-point atomic is on the path. */
int camo_inst_match(const int32_t* pred_labels, const int32_t* gt_labels, int32_t N, int32_t H, int32_t W,
                    int32_t P, int32_t G,
                    const int64_t* pred_table, int32_t pred_table_rows,
                    const int32_t* thr_num, int32_t thr_den, int32_t T,
                    int32_t* inter, int32_t* pred_rows, int32_t* gt_area, int32_t* match, int32_t* gt_match, int32_t* counts,
                    void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
