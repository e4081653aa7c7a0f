/*
 * texgs_ingest.h -- the input stage of libtexgs.so (csrc/ingest.hip): what the reference's loaders do to a view's 8-bit files before
 * a loss sees them -- Pillow's `Image.resize`, the division by 255, the permute to [C,H,W], the alpha mask and its product, the
 * normal map's 2 v - 1, the Blender loader's composite over a background -- on the device, from the uploaded BYTES (a quarter of the
 * float image).  Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs_present.h: device pointers, caller-allocated, everything enqueued on `stream` (a hipStream_t passed as
 * void*), 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch,
 * so a refused call has changed nothing.  No atomics, no host wait, no readback, no host-to-device copy: two calls give the same bits.
 *
 * The arithmetic is a bit-exact contract (tests/ingest_ref.py states it in numpy): the resample is Pillow's 8-bit one -- tap tables
 * in IEEE double with one rounding per operation, 22-bit fixed-point taps, int32 sums; the decode is fp32 with one rounding per
 * operation and IEEE division; the composite is IEEE double.
 */
#ifndef TEXGS_INGEST_H
#define TEXGS_INGEST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_INGEST_BICUBIC 0          /* Pillow's default for Image.resize; support 2, a = -0.5 */
#define TEXGS_INGEST_BILINEAR 1         /* support 1 */
#define TEXGS_INGEST_BOX 2              /* support 0.5 */

#define TEXGS_INGEST_PRECISION_BITS 22  /* a tap is (int) (p * 2^22 -+ 0.5); a sum starts at 2^21 and is shifted right by 22 */
#define TEXGS_INGEST_MAX_KSIZE 129      /* taps per output index: a 32 x bicubic, 64 x bilinear or 128 x box reduction */
#define TEXGS_INGEST_MAX_SIDE 16384     /* of the source and of the result */

#define TEXGS_INGEST_SIGNED 1u          /* out_chw: v = (v * 2.0f) - 1.0f after the division (normal maps) */

/* One axis of Pillow's resample, in_size -> out_size (all of it IEEE double, one rounding per operation):
 *     scale = in / out;  fs = max(scale, 1.0);  support = filter_support * fs;  ksize = (int) ceil(support) * 2 + 1
 *     per output index xx:  center = (xx + 0.5) * scale;  ss = 1.0 / fs
 *         xmin = max((int) (center - support + 0.5), 0);  n = min((int) (center + support + 0.5), in) - xmin
 *         w[x] = filter((x + xmin - center + 0.5) * ss), x = 0 .. n-1;  ww = w[0] + w[1] + ... in index order
 *         p[x] = w[x] / ww (w[x] when ww == 0);  k[x] = (int) (p[x] < 0 ? p[x] * 4194304.0 - 0.5 : p[x] * 4194304.0 + 0.5)
 *     out[xx] = clamp((2097152 + sum_x k[x] * in[xmin + x]) >> 22, 0, 255)        int32, arithmetic shift
 * texgs_resize_ksize returns ksize, or 0 for an axis the library refuses (a size outside [1, TEXGS_INGEST_MAX_SIDE], an unknown
 * filter, ksize > TEXGS_INGEST_MAX_KSIZE).
 * texgs_resize_taps writes the tables of one axis: taps int32 [ksize, out_size] (TRANSPOSED: tap x of output xx is
 * taps[x * out_size + xx], 0 for x >= n) and bounds int32 [out_size, 2] = (xmin, n).  Both 4-byte aligned.  One launch. */
int32_t texgs_resize_ksize(int32_t in_size, int32_t out_size, int32_t filter);
int texgs_resize_taps(int32_t in_size, int32_t out_size, int32_t filter, int32_t* taps, int32_t* bounds, void* stream);

/* texgs_resize_u8: src uint8 [src_height, src_width, channels] (channels 1 or 3: Pillow's modes L and RGB) resampled to
 * [height, width, channels] as Pillow does it: the horizontal pass first, into a uint8 intermediate (clamped: that is part of the
 * result) and only over the source rows the vertical pass reads, then the vertical pass; a pass whose size does not change is
 * skipped, not run with unit taps.  The tap tables are built on the device, in `temp`.
 * The decode is fused into the last pass (the vertical one; the horizontal one when the height is unchanged; a pass of its own when
 * neither size changes).  With b the resized byte of pixel p, channel c -- any non-empty subset, each element written exactly once:
 *     out_u8   [height, width, channels]   b
 *     out_chw  [channels, height, width]   v = (float) b / 255.0f;  v = (v * 2.0f) - 1.0f with TEXGS_INGEST_SIGNED;
 *                                          v = v * mul[p] with mul
 *     out_mask [1, height, width]          b of channel 0 > 0 ? 1.0f : 0.0f
 * src, out_u8, out_chw, out_mask, mul and temp: 4-byte aligned (rows of src and out_u8 are dense: no row alignment is asked). */
typedef struct TexGSResize {
    const uint8_t* src;
    const float* mul;           /* [height, width], or NULL */
    uint8_t* out_u8;
    float* out_chw;
    float* out_mask;
    int32_t src_height;
    int32_t src_width;
    int32_t channels;           /* 1 or 3 */
    int32_t height;
    int32_t width;
    int32_t filter;             /* TEXGS_INGEST_BICUBIC / _BILINEAR / _BOX */
    uint32_t flags;             /* TEXGS_INGEST_SIGNED */
} TexGSResize;

/* Bytes of `temp` for texgs_resize_u8 (the tables of both axes and the intermediate); 0 for a call it would refuse for its sizes,
 * channels or filter -- and 4 when neither size changes (nothing is kept there, but temp must not be NULL). */
size_t texgs_resize_temp_bytes(int32_t src_height, int32_t src_width, int32_t channels, int32_t height, int32_t width, int32_t filter);
int texgs_resize_u8(const TexGSResize* r, void* temp, size_t temp_bytes, void* stream);

/* texgs_rgba_composite: rgba uint8 [height, width, 4] over a background -> out uint8 [height, width, 3], in IEEE double:
 *     n = b / 255.0;  arr = (n_c * n_a) + (bg_c * (1.0 - n_a));  out_c = (uint8_t) trunc(arr * 255.0)
 * bg_*: each in [0, 1] (so the product lies in [0, 255]).  1 <= height, width <= TEXGS_INGEST_MAX_SIDE; both pointers 4-byte aligned. */
int texgs_rgba_composite(const uint8_t* rgba, uint8_t* out, int32_t height, int32_t width, double bg_r, double bg_g, double bg_b,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_INGEST_H */
