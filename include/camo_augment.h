/* C ABI of the training augmentation on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * Camouflaged-object training recipes (SINet-V2's loader and what copies it) augment with a random flip, a random crop, a random
 * rotation of +-15 degrees and PIL's four ImageEnhance operations: brightness, contrast, colour, sharpness, each with a random factor.
 * camo_resize gives the fine-tuner the crop and the flip; camo_augment gives it the rest without a host image loop: packed uint8
 * sources of mixed sizes, as camo_resize takes them, go through ONE inverse affine map per image and, optionally, the four
 * enhancements, into a dense [N, Ho, Wo, C] batch, uint8 or fp32 in [0, 1].
 * PARITY UNPINNED: the text below is the definition; it is restated in numpy in tests/augment_ref.py, which the kernels are tested
 * against for equality.  The definition is in exact integer arithmetic: PIL's enhancements in floating point agree with it within one
 * grey level each (tests/test_augment.py), and the four in sequence are not compared: single-level differences grow to about ten
 * levels through the sharpness extrapolation on noise, which is why the definition is the integers and not PIL.
 *
 * Device pointers only, enqueue-only on `stream` (no allocation, no synchronisation), 0 = ok / negative CAMO_E_* as in
 * camo_fusion.h; every check of a pointer or a scalar runs on the host before the first launch.  The ABI version is that of
 * camo_fusion.h.  All sums are integers (the one accumulation across blocks is a 64-bit integer atomic), so the result does not depend
 * on the order of accumulation: two calls give the same bytes, and a batch gives the bytes of its images taken one by one.
 *
 * THE TABLE.  `table` is device memory, int64 [N, CAMO_AUG_FIELDS], one row per image; offsets and strides count bytes from `src`:
 *    0 src_off          1 src_H            2 src_W            3 src_row_stride   4 src_pix_stride   5 src_ch_stride
 *    6 clip_y0          7 clip_x0          8 clip_h           9 clip_w             (the part of the source that may be read)
 *   10 a00   11 a01   12 b0   13 a10   14 a11   15 b1                              (the inverse map, Q16)
 *   16 border (0 constant, 1 replicate at the clip box's edge)
 *   17 fill (byte c of the constant in bits 8c .. 8c+7)
 *   18 k_brightness    19 k_contrast      20 k_colour        21 k_sharpness        (Q8, 0 .. 1024, 256 = unchanged; read only with enhance = 1)
 *   22, 23 reserved, must be zero
 * Channel c of source pixel (y, x) is byte src_off + y src_row_stride + x src_pix_stride + c src_ch_stride.  The destination is dense:
 * channel c of pixel (dy, dx) of image i is element ((i Ho + dy) Wo + dx) C + c of `dst`, which holds N Ho Wo C elements.
 *
 * THE MAP.  Let F = 16.  For destination pixel (dy, dx)
 *     X = a00 (2 dx + 1) + a01 (2 dy + 1) + b0,      Y = a10 (2 dx + 1) + a11 (2 dy + 1) + b1
 * in int64, in units of 2^-F source pixels in index space (index j sits at j 2^F).  All divisions and shifts below are floors, also of
 * negative values.
 *   NEAREST   one tap (floor((Y + 2^(F-1)) / 2^F), floor((X + 2^(F-1)) / 2^F)) of weight 1, den = 1.
 *   BILINEAR  ix = floor(X / 2^F), wx1 = X - ix 2^F, wx0 = 2^F - wx1, likewise in y; the taps are (iy, ix), (iy, ix + 1), (iy + 1, ix),
 *             (iy + 1, ix + 1) with the weight products wy wx, den = 2^32.
 * A tap outside the clip box reads the fill byte of its channel when border = 0, and the source at the tap clamped into the box when
 * border = 1.  num = sum wy wx p in int64.  With enhance = 0 the output is that of camo_resize:
 *     u8 = (2 num + den) / (2 den),           fp32 = (float)((double)num / (double)(255 den)).
 * An axis-aligned map (a01 = a10 = 0, a00 = +-cw 2^15 / Wo, b0 = (x0 - 1/2) 2^16 or, mirrored, (x0 + cw - 1/2) 2^16) with the crop as
 * the clip box and border 1 has exactly camo_resize's taps where cw 2^15 / Wo is an integer, and then gives camo_resize's bytes.
 * With enhance = 1 the u8 value is taken first and goes through THE ENHANCEMENTS; the fp32 output is then (float)((double)v / 255.0).
 * The enhancement with every factor 256 leaves the u8 image as it is, so its fp32 output is the ROUNDED byte over 255: NOT the same
 * fp32 bytes as enhance = 0, which divides the unrounded num.
 *
 * THE ENHANCEMENTS (enhance = 1, C = 3).  PIL's ImageEnhance restated in integers: brightness, contrast, colour, sharpness, in that
 * order, on the warped u8 image of P = Ho Wo pixels.
 *     blend(deg, v, k) = clamp(floor((deg (256 - k) + v k + 128) / 256), 0, 255)       per channel; 256 - k may be negative
 *     L(p) = (19595 R + 38470 G + 7471 B + 32768) >> 16                                 the luma of a pixel
 *   brightness  v <- blend(0, v, k_brightness)
 *   contrast    S = sum of L over the image after brightness, m = floor((2 S + P) / (2 P)), v <- blend(m, v, k_contrast)
 *   colour      v <- blend(L(p), v, k_colour), L of the pixel as it now is
 *   sharpness   s = the sum of the pixel's 3 x 3 neighbourhood + 4 times the pixel, per channel, sm = floor((2 s + 13) / 26); a pixel in
 *               row 0 or Ho - 1 or in column 0 or Wo - 1 has sm = itself, so an image with a side below 3 is unchanged;
 *               v <- blend(sm, v, k_sharpness)
 *
 * ROW VALIDITY.  The table is on the device, so the host cannot check it; the kernel checks every row before any read.  A row is good
 * when: src_H, src_W, clip_h, clip_w are in [1, CAMO_RSZ_MAX_SIDE]; clip_y0, clip_x0 >= 0 and the clip box lies inside the source; the
 * three strides are >= 1; src_off >= 0; the largest byte index of the source footprint (all src_H x src_W pixels, C channels) is below
 * src_elems, taken without overflow; |a_ij| <= 2^30 and |b_i| <= 2^46, so |X|, |Y| < 2^47; border is 0 or 1; fill is in [0, 2^32); with
 * enhance = 1 every k is in [0, 1024]; fields 22 and 23 are 0.  A good row gets status[i] = 0.  Any other row gets status[i] = 1, reads
 * NOTHING and leaves zeros in its whole destination image.  status is written with ordinary stores: every block of an image stores
 * the same value.  Nothing is ever read or written outside src, dst, table, status and ws.
 *
 * LAUNCHES.  enhance = 0: ONE launch, camo_resize's geometry: grid (ceil(Ho Wo / 1024), N), 256 threads, four destination pixels a
 * thread, a wave's lanes along a destination row; the taps are computed per thread from the integers above, there are no tap tables in
 * memory, and interleaved bytes are fetched as camo_resize fetches them.  enhance = 1: THREE launches: the N luma sums in ws are
 * cleared; the same warp kernel applies brightness, stores the image as one 32-bit word per pixel in ws and adds the block's luma sum
 * with one 64-bit integer atomic; then one block per 32 x 32 tile recomputes contrast and colour for the tile and a halo of one pixel
 * into LDS, takes the 3 x 3 sums there and stores dst.  The workspace may arrive dirty.  camo_augment_workspace_bytes is 0 with
 * enhance = 0 (ws may then be null) and 0 for arguments the call would refuse.
 *
 * Needs non-null src, dst, table, status (an fp32 dst 4-byte aligned, table 8-byte, status 4-byte); 1 <= N <= CAMO_RGD_MAX_IMAGES;
 * 1 <= C <= CAMO_RSZ_MAX_CHANNELS; Ho, Wo in [1, CAMO_RSZ_MAX_SIDE]; filter CAMO_RSZ_NEAREST or CAMO_RSZ_BILINEAR; dst_type CAMO_RSZ_U8
 * or CAMO_RSZ_F32; enhance 0 or 1, and C = 3 with enhance = 1; src_elems >= 1; with enhance = 1 a 256-byte aligned ws of at least
 * camo_augment_workspace_bytes: otherwise CAMO_E_ARG.
 *
 * NOT BUILT: fp32 sources; an AREA filter (a crop that shrinks more than 2 x aliases exactly as camo_resize's bilinear does); shear
 * (the six integers can state one, the Python side draws none); SINet's pepper noise on the ground truth; enhancement of images with
 * C != 3. */
#ifndef CAMO_AUGMENT_H
#define CAMO_AUGMENT_H
#include <stddef.h>
#include <stdint.h>
#include "camo_resize.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_AUG_FIELDS 24
#define CAMO_AUG_FRAC_BITS 16       /* F: the map's fixed point */
#define CAMO_AUG_MAX_FACTOR 1024    /* the largest k: an enhancement factor of 4 */
#define CAMO_AUG_TILE 32            /* the side of the enhancement's tile */

size_t camo_augment_workspace_bytes(int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t enhance);
int camo_augment(const uint8_t* src, int64_t src_elems, void* dst, int32_t dst_type,
                 const int64_t* table, int32_t N, int32_t C, int32_t Ho, int32_t Wo,
                 int32_t filter /* CAMO_RSZ_NEAREST | CAMO_RSZ_BILINEAR */, int32_t enhance /* 0 | 1 */,
                 int32_t* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
