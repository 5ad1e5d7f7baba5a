/* C ABI of the object instances of a predicted mask on MI355X, exported by the same libcamo_fusion.so as
 * include/camo_fusion.h (error text: camo_last_error()).
 *
 * Stands behind the first things a user asks of a camouflaged-object mask: how many objects there are, each one's box, size, centre
 * and confidence, and a mask without the specks and pinholes a per-superpixel paint leaves.  camo_instances binarises a probability
 * map, optionally fills the holes, labels the connected components, drops the small ones, numbers the rest in reading order and
 * sums a small integer table per component.  The device sums integers only and a component's root is its smallest pixel index, so
 * every output byte is a function of the inputs alone (two calls give the same bytes, a batch gives the rows of its images one by
 * one); the ratios -- centroid, score -- are taken from the integers in float64 on the host (camouflage_multimodal_amd/instances.py).
 * PARITY UNPINNED: the reference has no instance extraction and scipy.ndimage / cv2 are not part of this package, so their
 * conventions are not pinned.  The text below is the definition; it is restated in numpy, by flood fill, in tests/instances_ref.py,
 * which the kernels are tested against byte for byte.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_INSTANCES_H
#define CAMO_INSTANCES_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_detect.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_INST_FIELDS 8          /* int64 per instance row */
#define CAMO_INST_COUNTS 4          /* int32 per image */
#define CAMO_INST_MAX_ROWS (1 << 24)   /* N * max_instances */

/* Bytes of camo_instances' workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_instances_workspace_bytes(int32_t N, int32_t H, int32_t W);

/* The instances of an image batch in EIGHT launches, ELEVEN with fill_holes (all grids over the whole batch; the count does not
 * depend on N).  pred and pred_image_stride are exactly as for camo_seg_counts: image i's [H, W] plane starts at
 * pred + i * pred_image_stride floats (one channel of a [N, C, H, W] map is read in place).  ws: workspace of
 * camo_instances_workspace_bytes(N, H, W) bytes, 256-byte aligned.  Per image:
 *   1. Binarise.  A pixel is foreground when pred > threshold, compared in fp32; a NaN is background.
 *   2. Fill holes, when fill_holes != 0.  The background is labelled with the COMPLEMENTARY connectivity (4 when connectivity == 8,
 *      8 when connectivity == 4); a background component with no pixel in row 0, row H - 1, column 0 or column W - 1 is a hole, and
 *      all of a hole's pixels become foreground.
 *   3. Label the foreground of the (filled) mask with `connectivity`, 4 (edge neighbours) or 8 (edge and corner neighbours).
 *   4. Drop small components.  A component of fewer than min_area pixels (min_area >= 0) becomes background; area == min_area is kept.
 *   5. Number the kept components 1 .. K in the row-major order of each component's first pixel.
 *   6. labels int32 [N, H, W]: 0 on background, the id elsewhere -- all K ids, those above max_instances included.
 *   7. clean uint8 [N, H, W]: 1 where labels > 0, else 0.
 *   8. table int64 [N, max_instances, CAMO_INST_FIELDS]: the row of id k (k - 1 < max_instances) is
 *        (area, x0, y0, x1, y1, Sx, Sy, Sq)
 *      -- the pixel count, the inclusive bounding box (columns x0 .. x1, rows y0 .. y1), the sums of the column and of the row
 *      indices, and the sum over the component's pixels of q, the 8-bit quantisation of camo_seg_measures.h,
 *      q = (int) rintf(fminf(fmaxf(pred, 0.f), 1.f) * 255.0f) with a NaN giving 0; filled hole pixels are included (with their own q).
 *      Rows past K are zero: the call writes the whole table.
 *   9. counts int32 [N, CAMO_INST_COUNTS] = (K, the components dropped as small, the holes filled, the pixels of clean).
 * Needs 1 <= N <= CAMO_RGD_MAX_IMAGES, H, W >= 1, H * W <= CAMO_RGD_MAX_IMAGE_PIXELS, N * H * W <= CAMO_RGD_MAX_PIXELS,
 * connectivity 4 or 8, min_area >= 0, 1 <= max_instances, N * max_instances <= CAMO_INST_MAX_ROWS, pred_image_stride >= H * W, a finite
 * threshold, no null pointer, table 8-byte aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise CAMO_E_ARG.
 * What ws and the four outputs hold on entry is unspecified; every element of labels, clean, table and counts is written.
 *
 * 32 x 32 tiles are labelled in LDS by union-find, tile borders joined with agent-scope atomicMin on the larger root (parents only
 * decrease: the root is the smallest index whatever the order), never across an image's edge.  The statistics combine runs of equal
 * id inside a wave and an id's runs inside the block (LDS) before they reach memory, with 32- and 64-bit INTEGER atomics only: no
 * floating-point atomic is on the path.
 *
 * The ratios are not part of the ABI; per row the Python surface takes, in float64 from the exact integers,
 *   centroid = (Sx / area, Sy / area),  score = Sq / (255 area). */
int camo_instances(const float* pred, int64_t pred_image_stride, float threshold, int32_t N, int32_t H, int32_t W,
                   int32_t connectivity, int32_t min_area, int32_t fill_holes, int32_t max_instances,
                   int32_t* labels, uint8_t* clean, int64_t* table, int32_t* counts,
                   void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
