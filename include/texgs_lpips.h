/*
 * texgs_lpips.h -- the LPIPS-VGG entry points of libtexgs.so (csrc/lpips.hip): a 3x3 convolution as an implicit GEMM on the matrix
 * cores and the per-layer LPIPS head.  texgs/lpips.py chains thirteen convolutions and five heads into the metric that the
 * reference's utils/metrics.py:49-58 takes from the `lpips` package.  Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is
 * unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.  No entry point waits on the host, reads anything back or allocates.
 */
#ifndef TEXGS_LPIPS_H
#define TEXGS_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_LPIPS_FP32 0            /* v_mfma_f32_32x32x2_f32: exact f32 products, a k-ordered f32 chain */
#define TEXGS_LPIPS_BF16X3 1          /* reserved: split-bf16 products; NOT built -- refused by name by every entry point */

#define TEXGS_CONV_TILE_H 8           /* output pixels of one workgroup: 8 rows of 32 */
#define TEXGS_CONV_TILE_W 32
#define TEXGS_CONV_CIN_STEP 8         /* input channels staged in LDS at a time */
#define TEXGS_CONV_K_STEP 72          /* = 9 taps x 8 channels: K = 9 Cin is padded with zero weights to a multiple of it */
#define TEXGS_CONV_COUT_TILE 64       /* output channels of one workgroup; the packed weights are padded with zero rows to it */
#define TEXGS_CONV_MAX_CHANNELS 512
#define TEXGS_CONV_MAX_BATCH 65535    /* the batch is the grid's z dimension */
#define TEXGS_LPIPS_ROW 8             /* f64 slots of one pair's row: 0-4 the layers' terms, 5 their sum, 6-7 reserved (never written) */
#define TEXGS_LPIPS_LAYERS 5
#define TEXGS_LPIPS_HEAD_MAX_BLOCKS 1024   /* partial sums per pair */

/* Bytes of `packed` for a weight set (a multiple of 16); 0, with the cause in texgs_last_error(), for an unsupported argument. */
size_t texgs_conv3x3_packed_bytes(int32_t Cin, int32_t Cout, int32_t precision);

/* w f32[Cout, Cin, 3, 3] (the torch layout) -> the matrix cores' A-operand order, once per weight set.  `packed` is 16-byte
 * aligned.  Within a chunk of 8 input channels the k order is tap-major (k = 8 tap + channel); channels past Cin and rows past Cout
 * hold zeros. */
int texgs_conv3x3_pack(const float* w, int32_t Cin, int32_t Cout, int32_t precision, void* packed, void* stream);

/* y f32[B, Cout, Ho, Wo] = act(conv3x3(pad1(in(x))) + bias), x f32[B, Cin, H, W]; stride 1, zero padding 1; ONE launch.
 *   in(x)    = x * in_scale[c] + in_shift[c] per element when the two are given (both or neither), then, with pool_in, the 2x2 /
 *              stride-2 / floor-mode max-pool of that: Ho = H / 2, Wo = W / 2 and an odd last row or column is dropped.  Without
 *              pool_in Ho = H, Wo = W.
 *   pad1     pads in(x) with ZEROS: a tap outside the (pooled) image contributes 0, not in_shift.
 *   act      = max(., 0) when relu, else the identity.
 * x and y may be views into larger buffers: x_row, x_chan, x_img are the distances, in floats, from a row, a channel plane and an
 * image of x to the next (columns are adjacent), y_row, y_chan, y_img those of y.  All three of a tensor 0 means dense
 * (W, H W, Cin H W for x; Wo, Ho Wo, Cout Ho Wo for y); otherwise row >= the width, chan >= rows x row, img >= channels x chan.
 * Nothing outside the H x W (Ho x Wo) elements of each plane is read (written).
 * Limits: 1 <= Cin <= 512, Cout a multiple of 16 up to 512, Ho, Wo >= 1, 1 <= B <= 65535, B Ho Wo < 2^31, fewer than 2^24 tiles of
 * TEXGS_CONV_TILE_H x TEXGS_CONV_TILE_W output pixels per image (the launch's limit), B x img < 2^62 floats;
 * x, y, bias, in_scale, in_shift 4-byte aligned, packed 16-byte aligned.  Anything else is refused by name.
 * A tile of output pixels never spans two images and its arithmetic does not depend on B or on the slot: an image's output has the
 * same bits wherever it sits in a batch.  No atomics: two calls give the same bits. */
typedef struct TexGSConv3x3 {
    const float* x;
    const void* packed;          /* texgs_conv3x3_pack(w, Cin, Cout, precision) */
    const float* bias;           /* f32[Cout] */
    const float* in_scale;       /* f32[Cin] or NULL */
    const float* in_shift;       /* f32[Cin] or NULL */
    float* y;
    int32_t B, Cin, Cout, H, W;  /* H, W: of x, before pooling */
    int32_t relu;                /* 0 / 1 */
    int32_t pool_in;             /* 0 / 1 */
    int32_t precision;           /* TEXGS_LPIPS_* */
    int64_t x_row, x_chan, x_img;        /* strides of x in floats; 0, 0, 0: dense */
    int64_t y_row, y_chan, y_img;        /* strides of y in floats; 0, 0, 0: dense */
} TexGSConv3x3;

int texgs_conv3x3(const TexGSConv3x3* d, void* stream);

/* One tapped layer of LPIPS.  f f32[2P, C, h, w]: slots 0 .. P-1 hold the first images' features, P .. 2P-1 their partners'.
 * Per pixel, in f32:  n0 = sqrt(sum_c f0_c^2), n1 likewise,  d = sum_c lin_c (f0_c / (n0 + 1e-10) - f1_c / (n1 + 1e-10))^2
 * (sums in channel order, one rounding per operation).  Per pair, in f64:  out[p][layer] = (sum_pixels d) / (h w), from per-block
 * partial sums added in a fixed order by one block: no atomics, two calls give the same bits, and swapping the two images too.
 * `out` is f64[P][TEXGS_LPIPS_ROW]; with layer == 4, out[p][5] = out[p][0] + ... + out[p][4] in that order from the stored values
 * (the call of layer 4 comes last).  Limits: 1 <= P <= 65535, 1 <= C <= 512, h, w >= 1, h w < 2^31, 0 <= layer <= 4;
 * f and lin 4-byte aligned, out and temp 8-byte aligned. */
typedef struct TexGSLpipsHead {
    const float* f;
    const float* lin;            /* f32[C] */
    double* out;                 /* f64[P][8] */
    void* temp;                  /* texgs_lpips_head_temp_bytes(P, h, w) bytes */
    int32_t P, C, h, w;
    int32_t layer;
} TexGSLpipsHead;

/* Bytes of TexGSLpipsHead.temp (8-byte aligned); 0 for an unsupported argument. */
size_t texgs_lpips_head_temp_bytes(int32_t P, int32_t h, int32_t w);

int texgs_lpips_head(const TexGSLpipsHead* d, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_LPIPS_H */
