/* C ABI of COCO polygon annotations on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * Instance ground truth ships as COCO annotation files whose "segmentation" is a list of polygons for every annotation that is not a
 * crowd.  camo_poly_decode paints such polygons into the int32 label map camo_inst_match takes as ground truth, as camo_rle_decode
 * (camo_rle.h) paints run-length annotations: nothing is rasterised on the host.  Reading the annotation file and flattening its
 * lists is host work and lives in camouflage_multimodal_amd/polygons.py.  The mask of a polygon is a function of the inputs alone:
 * the few floating-point operations are stated one by one, and the rest is integers (two calls give the same bytes, a batch gives the
 * rows of its images one by one).
 * PARITY UNPINNED: pycocotools is not part of this package.  The text below follows its rleFrPoly and rleMerge(..., intersect = 0)
 * operation for operation so that it can be pinned later; it is restated sequentially in numpy in tests/poly_ref.py, which the kernels
 * are tested against byte for byte.
 * OUT OF SCOPE: the iscrowd flag and IoU taken in the RLE domain.
 *
 * ORDER.  camo_rle.h's: pixel (y, x) of an [H, W] image has position p = x H + y.
 *
 * THE MASK OF ONE POLYGON of k >= 1 vertices (x_j, y_j), float64:
 *   1. Vertices.  X_j = (int)(5.0 * x_j + 0.5) and Y_j likewise: one double multiply, one double add, each rounded (not fused),
 *      C's conversion toward zero.
 *      X_k = X_0, Y_k = Y_0.
 *   2. The boundary points of edge j, from (xs, ys) = (X_j, Y_j) to (xe, ye) = (X_{j+1}, Y_{j+1}).  dx = |xe - xs|, dy = |ye - ys|,
 *      n_j = max(dx, dy) + 1 points, d = 0 .. n_j - 1.  flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye); when flip is set
 *      the two ends are swapped.  Then
 *        dx >= dy:  t = flip ? dx - d : d,  u = xs + t,  v = (int)(ys + s t + 0.5)  with s = (double)(ye - ys) / dx
 *        dx <  dy:  t = flip ? dy - d : d,  v = ys + t,  u = (int)(xs + s t + 0.5)  with s = (double)(xe - xs) / dy
 *      The division is correctly rounded; the product and the two sums are rounded once each -- NO fused multiply-add: an
 *      implementation must switch its compiler's contraction off (csrc/poly.hip does, by pragma and by flag) --; the conversion
 *      is toward zero.  An edge with dx = dy = 0 has the one point (xs, ys).
 *   3. Crossings.  Over the points of all edges in order, every consecutive pair (u', v'), (u, v) with u != u' -- the pair that
 *      joins the last point of an edge to the first of the next included -- is tested: with m = min(u, u') it counts when
 *      m mod 5 == 2 (mod of the floor) and x = (m - 2) / 5 lies in 0 .. W - 1; then y = clamp(ceil((min(v, v') - 2) / 5), 0, H)
 *      and position x H + y is toggled.  (The integer form of rleFrPoly's (xd + .5) / scale - .5, exact at these magnitudes.)  A
 *      toggle at H W has no effect.
 *   4. Position p < H W is foreground iff the number of toggles at positions <= p is odd (rleFrPoly's sort, difference and
 *      zero-count merge).
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  32- and 64-bit INTEGER atomics only.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_POLY_H
#define CAMO_POLY_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rle.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_POLY_MAX_ANNOTATIONS 65535    /* A */
#define CAMO_POLY_MAX_POLYGONS 65535       /* P */
#define CAMO_POLY_MAX_VERTICES (1 << 20)   /* V */
#define CAMO_POLY_MARGIN 1024              /* pixels a vertex may lie outside the image */
#define CAMO_POLY_MAX_PLANE_WORDS (1 << 28)   /* P * ceil(H W / 32) */

/* Bytes of camo_poly_decode's workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_poly_decode_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t A, int32_t P, int32_t V);

/* The label maps of A annotations of P polygons in FOUR launches (verdict and clear, toggle, scan, paint; the count does not depend
 * on N, A, P or V).  xy is double [V, 2]: the vertices (x, y) of all polygons back to back.  poly_off int32 [P + 1]: polygon q's
 * vertices are xy[poly_off[q] .. poly_off[q + 1]).  ann_poly_off int32 [A + 1]: annotation a owns polygons ann_poly_off[a] ..
 * ann_poly_off[a + 1] - 1.  ann_image int32 [A]: the image of annotation a; ann_value int32 [A]: the value it paints, >= 1.
 * ws: workspace of camo_poly_decode_workspace_bytes(N, H, W, A, P, V) bytes, 256-byte aligned.
 * PRECONDITIONS (the Python surface checks them; this entry point cannot without a copy): both offset arrays are non-decreasing
 * from 0 to V and to P, and the boundary points of all edges, the sum of n_j, number at most 2^28.  The device clamps every offset
 * into its array, so no index leaves an input array whatever the caller passed.
 *   5. The call clears labels int32 [N, H, W] to 0.  An annotation is the union of its polygons' masks: every foreground position
 *      p of annotation a gets max(current, ann_value[a]) at pixel (p % H, p / H) of image ann_image[a].  The largest value wins and
 *      no order matters: camo_rle_decode's rule, so maps of both calls combine with an elementwise max.
 *   6. ann_area int64 [A]: the pixels of the union of a's polygons, before the max with other annotations.  An annotation without
 *      a polygon is valid and has area 0.
 *   7. An annotation with ann_image outside 0 .. N - 1, with ann_value < 1, or with a polygon that has no vertex, a non-finite
 *      coordinate or a coordinate outside [-CAMO_POLY_MARGIN, W + CAMO_POLY_MARGIN] (x) / [-CAMO_POLY_MARGIN, H + CAMO_POLY_MARGIN]
 *      (y) writes nothing and gets ann_area[a] = -1.  The margin bounds an edge's length and so every kernel's running time.
 * Needs camo_instances' limits on N, H and W, 1 <= A <= CAMO_POLY_MAX_ANNOTATIONS, 0 <= P <= CAMO_POLY_MAX_POLYGONS (P = 0 when
 * every annotation is empty), 0 <= V <= CAMO_POLY_MAX_VERTICES, P * ceil(H W / 32) <= CAMO_POLY_MAX_PLANE_WORDS, no null pointer (xy
 * may be null when V == 0), xy and ann_area 8-byte aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise
 * CAMO_E_ARG.
 * What ws, labels and ann_area hold on entry is unspecified; every element of labels and ann_area is written.
 *
 * The workspace holds one bit-plane per polygon, a bit per position.  The first launch takes step 7 for every polygon (a wave each)
 * and clears the label maps and the planes; the second takes one wave per edge, lanes over d in strides of 64, each lane its point
 * and the one before from the closed form of step 2, and toggles with one 32-bit atomicXor per crossing (its spare blocks take the
 * annotations' verdicts and set ann_area to 0 or -1); the third, one block per polygon, turns the toggles into the mask with an
 * inclusive prefix-XOR over the plane; the fourth, one thread per (annotation, word), ORs the annotation's planes, adds the
 * popcounts into ann_area (one 64-bit atomicAdd a wave) and paints every set bit with a 32-bit atomicMax. */
int camo_poly_decode(const double* xy, int32_t V, const int32_t* poly_off, int32_t P,
                     const int32_t* ann_poly_off, const int32_t* ann_image, const int32_t* ann_value, int32_t A,
                     int32_t N, int32_t H, int32_t W, int32_t* labels, int64_t* ann_area,
                     void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
