/* C ABI of the image resampler on MI355X, exported by the same libcamo_fusion.so as include/camo_fusion.h (error
 * text: camo_last_error()).
 *
 * Stands between the data and every image entry point of the region-graph path: COD10K, CAMO, NC4K and CHAMELEON are 8-bit files,
 * each of its own size, the detector works at one fixed size (256 x 256 in the reference), and the benchmark tables are scored at
 * each ground truth's own size.  camo_resize resamples a whole ragged batch in ONE launch, in either direction: packed HWC bytes of
 * mixed sizes to a fixed [N, Ho, Wo, C] fp32 batch in [0, 1] (with a crop box and a flip per image: the augmentation of the
 * fine-tuner), planar fp32 maps back to each image's native size, 8-bit masks with the same boxes.
 * PARITY UNPINNED: cv2 and skimage are absent and the reference's resize call cannot be read, so the text below is the definition;
 * it is restated in numpy in tests/resize_ref.py, which the kernel is tested against.  The definition is in exact integer
 * arithmetic (u8 sources) or in a fixed order of exactly representable products (fp32 sources), so the tests compare for equality.
 *
 * Device pointers only, enqueue-only on `stream` (no workspace, no allocation, no synchronisation), 0 = ok / negative CAMO_E_* as
 * in camo_fusion.h; every check of a pointer or a scalar runs on the host before the launch.  The ABI version is that of
 * camo_fusion.h.  No atomics and no floating-point reduction across threads: two calls give the same bytes, and a batch gives the
 * images of its rows one by one.
 *
 * THE TABLE.  `table` is device memory, int64 [N, CAMO_RSZ_FIELDS], one row per image; offsets and strides count ELEMENTS of the
 * side's type (bytes for CAMO_RSZ_U8, floats for CAMO_RSZ_F32) from `src` / `dst`:
 *    0 src_off          1 src_H            2 src_W            3 src_row_stride   4 src_pix_stride   5 src_ch_stride
 *    6 crop_y0          7 crop_x0          8 crop_h           9 crop_w          10 flip (bit 0 mirrors columns, bit 1 mirrors rows)
 *   11 dst_off         12 dst_H           13 dst_W           14 dst_row_stride  15 dst_pix_stride  16 dst_ch_stride
 *   17 reserved, must be zero
 * Channel c of source pixel (y, x) is element src_off + y src_row_stride + x src_pix_stride + c src_ch_stride; likewise the
 * destination.  Both sides are strided and ragged, so packed HWC, planar CHW and a channel slice of a larger tensor are all read
 * and written in place.
 *
 * PER AXIS.  An axis has crop origin c0, crop length cs and destination length D.  For destination index d let d' = D - 1 - d when
 * the axis is flipped, else d.  The axis gives taps (source index, integer weight) and their total T:
 *   NEAREST   one tap c0 + floor((2 d' + 1) cs / (2 D)), weight 1, T = 1.
 *   BILINEAR  (and an AREA axis with cs <= D)  n = (2 d' + 1) cs - D, i0 = floor(n / (2 D)), w1 = n - i0 2 D, w0 = 2 D - w1; taps
 *             c0 + clamp(i0, 0, cs - 1) with weight w0 and c0 + clamp(i0 + 1, 0, cs - 1) with weight w1, T = 2 D.  Pixel centres at
 *             half-integers, the border repeated AT THE CROP'S EDGE: the sampling rule of cv2.INTER_LINEAR and of
 *             F.interpolate(align_corners=False).
 *   AREA      with cs > D: pixel j of the crop, 0 <= j < cs, has weight w_j = min((d' + 1) cs, (j + 1) D) - max(d' cs, j D) where
 *             that is positive; its tap is c0 + j; T = cs.  The exact fractional-coverage box of cv2.INTER_AREA.
 *
 * PER PIXEL AND CHANNEL, u8 source.  num = sum_y sum_x wy wx p in int64, den = Ty Tx.
 *   fp32 output = (float)((double)num / (double)(255 den)): one double division, then one conversion.  (u8 -> f32 is the exact
 *                 value divided by 255.)
 *   u8 output   = (2 num + den) / (2 den) in integers: a half rounds up.
 * PER PIXEL AND CHANNEL, fp32 source (NEAREST and BILINEAR only).  The value is sum (double)(wy wx) (double)p over the one tap
 *   (NEAREST) or over the four taps (BILINEAR) in row-major order -- (y0, x0), (y0, x1), (y1, x0), (y1, x1) -- each add rounded
 *   once, then divided by (double)den and converted to float.  Every product is exact in double: with sides <= 8192, wy wx < 2^28
 *   and an fp32 value has 24 significant bits, so contracting a multiply and an add into an FMA cannot change a bit.
 * fp32 -> u8, and AREA with an fp32 source, are refused (CAMO_E_ARG).
 *
 * ROW VALIDITY.  The table is on the device, so the host cannot check it; the kernel checks every row before it touches memory.
 * A row is good when: src_H, src_W, crop_h, crop_w, dst_H, dst_W are in [1, CAMO_RSZ_MAX_SIDE]; crop_y0, crop_x0 >= 0 and the
 * crop lies inside the source; the six strides are >= 1; flip is in 0..3; field 17 is 0; both offsets are >= 0; the largest element
 * index of the source footprint (all src_H x src_W pixels, C channels) is below src_elems and that of the destination footprint
 * below dst_elems, both taken without overflow; dst_H dst_W <= max_dst_pixels.  A good row gets status[i] = 0.  Any other row
 * gets status[i] = 1 and reads NOTHING; zeros are stored over whatever elements of its stated destination lie inside
 * [0, dst_elems) -- when the destination's own fields (offset, sides, strides, the max_dst_pixels bound) are good, else nothing is
 * stored for it.  status is written with ordinary stores: every block of an image stores the same value.  Footprints of different
 * rows that overlap in dst are the caller's business: nothing is read or written outside the two buffers either way.
 *
 * LAUNCH.  ONE launch, grid = (ceil(max_dst_pixels / 1024), N), 256 threads; thread t of block b of image i produces destination
 * pixels b 1024 + t, + 256, + 512, + 768 in row-major order, all channels each, so a wave's lanes run along a destination row;
 * blocks past an image's own pixels leave after the status store.  Taps are computed per thread from the integers above; there are
 * no tap tables in memory.  The bytes of a u8 pixel with interleaved channels are fetched as one unaligned 32-bit load where those
 * four bytes lie inside [0, src_elems), byte by byte otherwise.
 *
 * Needs non-null src, dst, table, status (fp32 sides 4-byte aligned, table 8-byte, status 4-byte); 1 <= N <= CAMO_RGD_MAX_IMAGES;
 * 1 <= C <= CAMO_RSZ_MAX_CHANNELS; a known filter, known types and an allowed combination; 1 <= max_dst_pixels <=
 * CAMO_RSZ_MAX_SIDE^2; src_elems, dst_elems >= 1: otherwise CAMO_E_ARG. */
#ifndef CAMO_RESIZE_H
#define CAMO_RESIZE_H
#include <stddef.h>
#include <stdint.h>
#include "camo_rg_detect.h"
#ifdef __cplusplus
extern "C" {
#endif

#define CAMO_RSZ_FIELDS 18
#define CAMO_RSZ_MAX_SIDE 8192      /* every source, crop and destination side */
#define CAMO_RSZ_MAX_CHANNELS 4
#define CAMO_RSZ_NEAREST 0
#define CAMO_RSZ_BILINEAR 1
#define CAMO_RSZ_AREA 2
#define CAMO_RSZ_U8 0
#define CAMO_RSZ_F32 1

int camo_resize(const void* src, int64_t src_elems, int32_t src_type, void* dst, int64_t dst_elems, int32_t dst_type,
                const int64_t* table, int32_t N, int32_t C, int32_t filter, int64_t max_dst_pixels,
                int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
