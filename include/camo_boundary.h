/* C ABI of Boundary IoU on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error text:
 * camo_last_error()).
 *
 * Mask IoU grows with object area: a 40 x 40 square shifted by two pixels still has IoU 0.82, so a measure built on it barely sees
 * where a large object's contour lies.  Boundary IoU (Cheng, Girshick, Dollar, Berg, Kirillov, CVPR 2021) is the IoU of the two
 * BOUNDARY REGIONS -- an instance minus its erosion by d iterations of a 3 x 3 square, the image border counting as outside --
 * and Boundary AP is COCO's greedy matching on min(mask IoU, boundary IoU).  camo_boundary_labels turns a label map into the map
 * of its instances' boundary regions; camo_boundary_match is camo_inst_match (include/camo_inst_match.h) with that second pair of
 * maps.  Everything is integer arithmetic, so every output byte is a function of the inputs alone (two calls give the same bytes,
 * a batch gives the rows of its images one by one).  d is the caller's: the paper's is round(0.02 x image diagonal)
 * (camouflage_multimodal_amd/boundary.py, boundary_distance).
 * PARITY UNPINNED: the reference has no boundary measure and the Boundary IoU API (cv2.erode per annotation on the host) is not part
 * of this package, so its conventions are not pinned.  The text below is the definition; it is restated in numpy in
 * tests/boundary_ref.py, which the kernels are tested against byte for byte, and which is held there to
 * scipy.ndimage.binary_erosion on a zero-padded mask -- the API's mask_to_boundary.
 * Out of scope: overlapping ground-truth instances (a label map cannot hold them, as in camo_inst_match.h), iscrowd ignore
 * matching, the boundary F-measure with a distance tolerance, gradients through the erosion.
 *
 * Device pointers only (thr_num excepted: a HOST array), enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok /
 * CAMO_E_ARG as in camo_fusion.h; every argument check runs on the host before any launch.  The ABI version is that of
 * camo_fusion.h. */
#ifndef CAMO_BOUNDARY_H
#define CAMO_BOUNDARY_H
#include <stddef.h>
#include <stdint.h>
#include "camo_inst_match.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_BD_MAX_DISTANCE (1 << 12) /* d */
#define CAMO_BD_STRIP 64               /* rows of an image a block of the column pass takes */
#define CAMO_BD_ROW_FIELDS 6           /* int32 per predicted id in camo_boundary_match's pred_rows */
#define CAMO_BD_GT_FIELDS 2            /* int32 per ground-truth id in camo_boundary_match's gt_area */

/* Bytes of camo_boundary_labels' workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_boundary_labels_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t d);

/* The boundary regions of the instances of a label map, in TWO launches whatever N (both grids over the whole batch; one launch
 * when 2d + 1 exceeds a side).  labels and out are int32 [N, H, W] and must not overlap.  Per image and pixel (y, x), with
 * L = labels[y][x]:
 *   - L <= 0: out = 0;
 *   - otherwise out = 0 (interior) when the whole window [y - d, y + d] x [x - d, x + d] lies inside the image and every pixel of it
 *     has label L;
 *   - otherwise out = L (boundary).
 * A label <= 0 differs from every positive label, so an ignore region (-1) erodes its neighbours as background does.  Images do not
 * see each other, rows do not see each other's ends.  This is the instance minus d iterations of the 3 x 3 erosion of the instance
 * padded with one ring of zeros; every instance with a pixel keeps at least one boundary pixel.  A d larger than a side is legal
 * and makes every foreground pixel boundary.
 * Needs camo_instances' limits on N, H and W, 1 <= d <= CAMO_BD_MAX_DISTANCE, no null pointer, labels and out not overlapping, ws
 * 256-byte aligned and ws_bytes at least camo_boundary_labels_workspace_bytes(N, H, W, d): otherwise CAMO_E_ARG.  What out and ws hold
 * on entry is unspecified; every element of out is written.
 *
 * The erosion by a square is separable, and each pass works on RUNS of equal values, so a pixel costs the same whatever d:
 *   row pass     one wave per image row, 64 pixels a step.  Two ballots over the lanes that start a run give every lane the run
 *                it is in; a run that reaches the end of a step is carried to the next step of the same row, never past the
 *                row's end (the run is clipped to the row: that is what makes the border count as outside).  With the run
 *                [s, e): rowok = x - s >= d and e - 1 - x >= d, one byte per pixel in ws.
 *   column pass  over the key (L where rowok and L > 0, else none) a pixel is interior iff its vertical run of equal keys reaches d
 *                up and d down inside the image.  Threads sit on consecutive x, so every read and write is coalesced; a block takes
 *                a strip of CAMO_BD_STRIP rows.  The runs leave the strip, so a thread first counts the rows below the strip that
 *                continue its last row's key -- at most d of them, none when that key is none, which is the common case --,
 *                sweeps UP the strip and keeps one bit per row (the run reaches d down), does the same above the strip, and
 *                sweeps DOWN writing out.  The halo is read, never written, so strips do not depend on each other. */
int camo_boundary_labels(const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t d, int32_t* out,
                         void* ws, size_t ws_bytes, void* stream);

/* Bytes of camo_boundary_match's workspace; 0 when the arguments are not supported (camo_inst_match's limits). */
size_t camo_boundary_match_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t P, int32_t G, int32_t T);

/* camo_inst_match under the combined IoU, in SEVEN launches whatever N (clear, overlap, areas for each of the two tables; match).
 * pred_labels, gt_labels: the instance maps; pred_bd, gt_bd: their boundary maps (camo_boundary_labels of each, with one d), all
 * int32 [N, H, W].  The other inputs are camo_inst_match's.
 *   Tables.  inter is the overlap table of (pred_labels, gt_labels), inter_bd that of (pred_bd, gt_bd), both int32
 *     [N, P + 1, G + 1]; each table's areas are its own row and column sums, and a label out of range enters no cell.  Items 1 - 4
 *     and 7 of camo_inst_match.h apply unchanged; counts comes from the mask maps.
 *   Combined IoU.  For a pair with mask (i, u), u = area_p + area_g - i, and boundary (ib, ub), ub the same from inter_bd's sums,
 *     the combined IoU is the smaller of i / u and ib / ub, decided by i ub against ib u in 64 bits (every factor is at most 2^27).
 *     ub = 0 makes it 0 / 1; when the two are equal the mask fraction is the one carried.
 *   Greedy match.  Item 5 of camo_inst_match.h with the combined fraction I / U in the threshold test thr_den I >= thr_num[k] U
 *     and in "best" (I1 U2 > I2 U1, ties to the smaller id).  A candidate still needs area_g > 0 and i > 0.  Rank and score order
 *     are unchanged.  match int32 [N, T, P], gt_match int32 [N, T, G].
 *   pred_rows int32 [N, P, CAMO_BD_ROW_FIELDS] = (area_p, the 0-based rank, the ground-truth id of highest combined IoU among those
 *     with i > 0 -- 0 when there is none, ties to the smaller id --, the mask intersection with it, the boundary area of p, the
 *     boundary intersection with it).  gt_area int32 [N, G, CAMO_BD_GT_FIELDS] = (area, boundary area).
 * Needs what camo_inst_match needs, for all four maps and both tables: otherwise CAMO_E_ARG.  What ws and the outputs hold on entry
 * is unspecified; every element of inter, inter_bd, pred_rows, gt_area, match, gt_match and counts is written.
 *
 * The first six launches are camo_inst_match's own kernels; the match launch is its one-barrier-per-rank loop with the two
 * boundary area vectors beside the mask's in LDS (25 KB in all) and a second row read per candidate. */
int camo_boundary_match(const int32_t* pred_labels, const int32_t* gt_labels, const int32_t* pred_bd, const int32_t* gt_bd,
                        int32_t N, int32_t H, int32_t W, int32_t P, int32_t G,
                        const int64_t* pred_table, int32_t pred_table_rows,
                        const int32_t* thr_num, int32_t thr_den, int32_t T,
                        int32_t* inter, int32_t* inter_bd, int32_t* pred_rows, int32_t* gt_area, int32_t* match, int32_t* gt_match,
                        int32_t* counts, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
