/* C ABI of COCO run-length masks on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * Stands at the two ends of the instance path: camo_rle_runs turns the label maps camo_instances writes into the runs from which
 * COCO's run-length encoding (RLE: {"size": [h, w], "counts": "..."} of a results JSON) is read off, and camo_rle_decode paints the
 * counts of COCO annotations into a label map that camo_inst_match takes as ground truth.  Neither end copies a label map to the
 * host.  The string form of the counts (COCO's rleToString / rleFrString) is host work on a few integers per run and lives in
 * camouflage_multimodal_amd/rle.py.  Everything is integers, so every output byte is a function of the inputs alone (two calls give
 * the same bytes, a batch gives the rows of its images one by one).
 * PARITY UNPINNED: pycocotools is not part of this package, so its conventions are not pinned.  The text below is the definition; it
 * is restated in numpy in tests/rle_ref.py, which the kernels are tested against byte for byte.
 * Polygon annotations (COCO's frPoly) have a call of their own: camo_poly.h.  OUT OF SCOPE: the iscrowd flag and IoU taken in the RLE
 * domain.
 *
 * ORDER.  COCO flattens a mask column by column: pixel (y, x) of an [H, W] image has position p = x H + y, and a run continues
 * across the bottom of one column into the top of the next.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  32- and 64-bit INTEGER atomics only.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_RLE_H
#define CAMO_RLE_H
#include <stddef.h>
#include <stdint.h>
#include "camo_instances.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_RLE_MAX_ROWS (1 << 26)        /* N * R */
#define CAMO_RLE_MAX_ANNOTATIONS 65535     /* A */
#define CAMO_RLE_MAX_COUNTS (1 << 26)      /* total */

/* Bytes of camo_rle_runs' workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_rle_runs_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t R);

/* The runs of an image batch in THREE launches (count, scan, emit; all grids over the whole batch; the count does not depend on N).
 * labels is int32 [N, H, W], row-major as camo_instances writes it; R is the capacity.  ws: workspace of
 * camo_rle_runs_workspace_bytes(N, H, W, R) bytes, 256-byte aligned.  Per image:
 *   1. runs int32 [N, R, 2] holds (start, label) of every maximal run of equal label along p, background runs included, in
 *      increasing start; the first run starts at 0.  A run's length is the next run's start minus its own, and H W - start for the
 *      last.  Labels are compared as raw int32 values; any value is a label.
 *   2. counts int32 [N, 2] = (M, the number of runs in all; min(M, R), the number written).
 *   3. Rows past min(M, R) are zero: the call writes the whole array.
 * Needs camo_instances' limits on N, H and W, 1 <= R, N * R <= CAMO_RLE_MAX_ROWS, no null pointer, labels and counts 4-byte and runs
 * 8-byte aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise CAMO_E_ARG.
 * What ws, runs and counts hold on entry is unspecified; every element of runs and counts is written.
 *
 * The label map is row-major and the order is column-major, so the pixel pass is a transposition: a block loads a 64 x 64 tile and
 * the row above it with lanes along x, and reads it back from LDS with lanes along y.  A position is a head when p == 0 or its label
 * differs from position p - 1's; a ballot counts the heads of a column segment of 64 rows, one block per image takes the exclusive
 * prefix of the segment counts in column-major order, and the same tile body run again writes every head at its rank. */
int camo_rle_runs(const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t R,
                  int32_t* runs, int32_t* counts,
                  void* ws, size_t ws_bytes, void* stream);

/* Bytes of camo_rle_decode's workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_rle_decode_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t A, int32_t total);

/* The label maps of A annotations in TWO launches (clear and prefix, fill -- no fill when total == 0; the count does not depend on
 * N or A).  cnts is int32 [total]: the counts of the A annotations back to back, each in COCO order -- the first count is
 * background, the second foreground, and so on in turn.  ann_off int32 [A + 1]: annotation a's counts are cnts[ann_off[a] .. ann_off[a + 1]);
 * PRECONDITION (the Python surface checks it; this entry point cannot without a copy): ann_off is non-decreasing from 0 to total.
 * ann_image int32 [A]: the image of annotation a; ann_value int32 [A]: the value it paints, >= 1.  ws: workspace of
 * camo_rle_decode_workspace_bytes(N, H, W, A, total) bytes, 256-byte aligned.
 *   1. The call clears labels int32 [N, H, W] to 0.
 *   2. For annotation a, every position p < H W of its foreground runs -- the 2nd, 4th, ... of its counts -- gets
 *      max(current, ann_value[a]) at pixel (p % H, p / H) of image ann_image[a].  The largest value wins, so the result does not
 *      depend on any order; ids 1 .. K in list order mean "later wins".
 *   3. ann_sum int64 [A]: the sum of a's counts.  The caller compares it with H W; the device writes nothing at or past H W
 *      whatever the counts say.
 *   4. An annotation with a negative count, with ann_image outside 0 .. N - 1 or with ann_value < 1 writes nothing and gets
 *      ann_sum[a] = -1.
 * Needs camo_instances' limits on N, H and W, 1 <= A <= CAMO_RLE_MAX_ANNOTATIONS, 0 <= total <= CAMO_RLE_MAX_COUNTS, no null pointer
 * (cnts may be null when total == 0), ann_sum 8-byte aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise
 * CAMO_E_ARG.
 * What ws, labels and ann_sum hold on entry is unspecified; every element of labels and ann_sum is written.
 *
 * The first launch clears labels and, one block per annotation, writes the start position of every run (the exclusive prefix of
 * the counts, taken in 64 bits and clamped to H W) into the workspace with ann_sum and the verdict of 4.  The second is the
 * SCATTER form: 16 consecutive lanes per count find the count's annotation by binary search in ann_off, leave when the count is a
 * background one, and walk the run's positions with a 32-bit atomicMax each. */
int camo_rle_decode(const int32_t* cnts, int32_t total, const int32_t* ann_off, const int32_t* ann_image, const int32_t* ann_value,
                    int32_t A, int32_t N, int32_t H, int32_t W,
                    int32_t* labels, int64_t* ann_sum,
                    void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
