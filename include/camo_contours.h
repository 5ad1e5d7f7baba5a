/* C ABI of instance contours on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * The instance path reads COCO ground truth as run-length masks (camo_rle.h) and as polygons (camo_poly.h) and wrote only the
 * first.  camo_contours turns the label maps camo_instances writes into the closed outlines of every id, with the vertices on the
 * integer corners of the pixels, so that a polygon painted back by camo_poly_decode covers exactly the pixels it was traced from.  No
 * label map is copied to the host.  Grouping the rings by id, telling outlines from holes and writing the annotation file is host
 * work on a few integers per ring and lives in camouflage_multimodal_amd/contours.py.  Everything is integers, so every output
 * byte is a function of the inputs alone (two calls give the same bytes, a batch gives the rows of its images one by one).
 * PARITY UNPINNED: neither OpenCV nor pycocotools is part of this package, so no convention of theirs is pinned.  The text below is
 * the definition; it is restated sequentially in numpy in tests/contours_ref.py, which the kernels are tested against byte for byte.
 * OUT OF SCOPE: simplifying an outline (dropping vertices within a tolerance), the iscrowd flag.
 *
 * GEOMETRY.  labels is int32 [N, H, W], row-major as camo_instances writes it.  A value > 0 is an id; every other value, and
 * everything outside the image, is background.  Corners are the lattice points (x, y) with 0 <= x <= W and 0 <= y <= H; the pixel
 * of row y and column x has the corners (x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1).
 *   A CRACK is a side of a pixel with id L whose neighbour across that side has another value.  It is directed so that the pixel
 *   lies on its right (y points down):
 *     side 0, top:     (x, y)         -> (x + 1, y)          heading (+1, 0)
 *     side 1, right:   (x + 1, y)     -> (x + 1, y + 1)      heading (0, +1)
 *     side 2, bottom:  (x + 1, y + 1) -> (x, y + 1)          heading (-1, 0)
 *     side 3, left:    (x, y + 1)     -> (x, y)              heading (0, -1)
 *   A crack's index is e = 4 (y W + x) + s.  A side between two different ids carries two cracks, one for each id.
 *
 * THE SUCCESSOR of crack (p, s) of id L with heading d.  b is the pixel after p along d, a the pixel to the left of b (the left of
 * heading (dx, dy) is (dy, -dx)).
 *   1. a has L, and b has L or connectivity == 8:  turn left, to crack (a, (s + 3) mod 4).
 *   2. otherwise, b has L:                         straight on, to crack (b, s).
 *   3. otherwise:                                  turn right, to crack (p, (s + 1) mod 4).
 * "a has L and b has not" is the saddle: connectivity 8 crosses to the diagonal pixel, connectivity 4 stays with its own.
 * Connectivity has no other effect.  Every crack has one successor and one predecessor; the cycles of this map are the RINGS.
 *
 * A RING.  Its first crack is the one of smallest index.  Its vertices are the start corners of the cracks whose predecessor has
 * another side number, in ring order from the first crack on (the first crack itself need not start at a vertex: a hole whose top
 * row is wider than one pixel starts in the middle of an edge).  Its a2 is the sum of x0 y1 - x1 y0 over its cracks (x0, y0) ->
 * (x1, y1), in int64: positive for an outline, negative for a hole, and the a2 of an id's rings sum to twice its pixel count.
 * The rings of an image are ordered by first crack.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / CAMO_E_ARG as in camo_fusion.h; every
 * argument check runs on the host before any launch.  32- and 64-bit INTEGER atomics only.  The ABI version is that of camo_fusion.h. */
#ifndef CAMO_CONTOURS_H
#define CAMO_CONTOURS_H
#include <stddef.h>
#include <stdint.h>
#include "camo_instances.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_CONTOUR_RING_FIELDS 5             /* int64 per ring row */
#define CAMO_CONTOUR_COUNTS 6                  /* int32 per image */
#define CAMO_CONTOUR_MAX_CRACKS (1 << 26)      /* N * C */
#define CAMO_CONTOUR_MAX_RINGS (1 << 24)       /* N * R */
#define CAMO_CONTOUR_MAX_VERTICES (1 << 26)    /* N * V */
/* The largest C of the LDS form.  A crack's link state is ONE 32-bit word of two 16-bit halves -- (ring head so far, successor), then
 * (vertices to the ring's end, successor): every position is below 2^16, the end-of-chain mark 0xFFFF is none of them and a vertex
 * count fits as well.  A round reads one buffer of such words and writes a second, so a crack takes 8 bytes: 2^14 cracks are 128 KiB
 * of the 160 KiB of a CU's LDS, and 2^15 would need 256 KiB.  So 2^14 is the largest power of two that fits. */
#define CAMO_CONTOUR_LDS_CRACKS (1 << 14)

/* Bytes of camo_contours' workspace; 0 when the arguments are not supported (the limits below). */
size_t camo_contours_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t R, int32_t V);

/* The rings of an image batch.  C, R and V are the capacities in cracks, rings and vertices per image.  ws: workspace of
 * camo_contours_workspace_bytes(N, H, W, C, R, V) bytes, 256-byte aligned.  Per image, with E its cracks, M its rings and T its
 * vertices:
 *   1. rings int64 [N, R, 5] holds (label, first crack, offset of its first vertex in the image's xy, vertex count, a2) of ring r
 *      in row r, for r < min(M, R).
 *   2. xy int32 [N, V, 2] holds the vertices (x, y) of the rings back to back in ring order; vertex t < min(T, V) is in row t.
 *   3. counts int32 [N, 6] = (E, M, T, cracks taken, rings written = min(M, R), vertices written = min(T, V)).
 *   4. An image with E > C takes no crack: M = T = 0 and cracks taken = 0 for it, nothing else is written, and E says what capacity
 *      a second call needs.  Otherwise cracks taken = E.
 *   5. Rows and vertices past what is written are zero: the call writes the whole of all three arrays.  A ring whose row is not
 *      written (r >= R) still has its vertices in xy, and a ring whose vertices do not all fit still has its row.
 * Needs camo_instances' limits on N, H and W, connectivity 4 or 8, 1 <= C <= 4 H W, 1 <= R, 1 <= V, N * C <= CAMO_CONTOUR_MAX_CRACKS,
 * N * R <= CAMO_CONTOUR_MAX_RINGS, N * V <= CAMO_CONTOUR_MAX_VERTICES, no null pointer, labels and counts 4-byte, xy and rings 8-byte
 * aligned, ws 256-byte aligned and ws_bytes at least the workspace size: otherwise CAMO_E_ARG.
 * What ws, rings, xy and counts hold on entry is unspecified; every element of rings, xy and counts is written.
 *
 * THE SCHEDULE follows from the arguments alone; the launch count depends on C only, never on N or on what the maps hold, and no
 * block waits for another block.  With K = ceil(log2 C):
 *   count    per 256 consecutive pixels: every pixel's 4-bit crack mask and its offset within the block (one 16-bit word), the block's
 *            crack count; the blocks of an image also clear its rows of rings and xy
 *   scan     one block per image: exclusive prefix of the block counts, E, and the verdict of 4
 *   link     per pixel again: a crack's position is its block's prefix plus its pixel's offset plus the set mask bits below its own
 *            -- compact order is increasing crack index --; its successor's position, its index, and its SUCCESSOR's is-vertex bit
 *            (the successor has another side number) go to the workspace
 *   heads    min-doubling, K rounds of m = min(m, m[next]), next = next[next], from one buffer into the other: K rounds always
 *            suffice because a ring is never longer than the cracks taken.  m ends as the position of the ring's first crack
 *   places   the chain is cut before the head (a crack whose successor is its head ends it); K rounds of s = s + s[next],
 *            next = next[next] give every crack the vertices from it to the ring's end, so a vertex crack's place in its ring is
 *            s[head] - s[crack]
 *   rank     one block per image: heads (m == own position) ranked by a scan over compact order, the rings' vertex counts scanned
 *            to offsets, the table rows and counts written
 *   emit     per crack: a vertex crack writes its start corner at its ring's offset plus its place; every crack adds its term to
 *            its ring's a2 with a 64-bit integer atomic add, summed first over the runs of equal ring inside a wave
 * LDS form, C <= CAMO_CONTOUR_LDS_CRACKS: heads and places run in ONE launch, one block of 1024 threads per image with the link
 * state in LDS (above), a round reading one buffer and writing the other, one barrier a round, ceil(log2 E) rounds each.
 * SIX launches: count, scan, link, doubling, rank, emit.
 * Global form, C > CAMO_CONTOUR_LDS_CRACKS: every round of heads and of places is a launch over the whole batch on (value, next)
 * pairs in global memory; the first round of each reads the link pass's arrays, so neither needs a launch to set up.  5 + 2 K
 * launches.
 * C < 4 holds no ring (a ring has at least four cracks): TWO launches, count and scan. */
int camo_contours(const int32_t* labels, int32_t N, int32_t H, int32_t W, int32_t connectivity,
                  int32_t C, int32_t R, int32_t V,
                  int64_t* rings, int32_t* xy, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
