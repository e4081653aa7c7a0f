/*
 * texgs_present.h -- the output stage of libtexgs.so (csrc/present.hip): what the callers of the rasterizer do to its maps before a
 * person looks at them -- clamp, composite over a background, quantise to 8 bits, interleave for a viewer, colour a depth map, lay a
 * cubemap out as a cross -- each as ONE streaming pass.  Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is unchanged); plain C99,
 * nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.  No atomics, no host wait, no readback: two calls give the same bits.
 *
 * The arithmetic is a bit-exact contract (tests/present_ref.py states it in numpy float32): fp32, every operation rounded once, no
 * fused multiply-add, IEEE division.  P = height * width, 1 <= P < 2^31.
 */
#ifndef TEXGS_PRESENT_H
#define TEXGS_PRESENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_PRESENT_PIXELS_PER_THREAD 4           /* a thread assembles 4 pixels into whole dwords */
#define TEXGS_PRESENT_PIXELS_PER_WORKGROUP 1024     /* 256 threads of 4 pixels per pass of the grid-stride loop */
#define TEXGS_PRESENT_MAX_WORKGROUPS 2048           /* the grid's cap; also the largest number of depth-range partials */

#define TEXGS_PRESENT_AFFINE 1u         /* v = 0.5f * (v + 1.0f) first (normal maps): the sum, then the product */
#define TEXGS_PRESENT_COMPOSITE 2u      /* v = (v * a) + (bg[c] * (1.0f - a)) after the clamp; needs alpha */
#define TEXGS_PRESENT_SWAP_RB 4u        /* out_u8 only: channel order b, g, r (cv2.imwrite) */

/* texgs_present, per pixel p and output channel c in 0..2 (a one-channel source is broadcast):
 *     v = src[min(c, channels - 1) * P + p]
 *     v = 0.5f * (v + 1.0f)                      with TEXGS_PRESENT_AFFINE
 *     v = min(max(v, 0), 1)                      a NaN stays NaN (torch.clamp)
 *     v = (v * a) + (bg[c] * (1.0f - a))         with TEXGS_PRESENT_COMPOSITE, a = alpha[p]
 * Outputs, any non-empty subset, each element written exactly once:
 *     out_u8   [H, W, u8_channels]  (uint8_t) trunc(v * 255.0f): below 0 and NaN give 0, 256 and above give 255; channel 3 is 255
 *     out_hwc4 [H, W, 4] f32        v, v, v, 1.0f         (a viewer's upload format)
 *     out_chw  [3, H, W] f32        v
 * src, alpha, out_chw: 4-byte aligned.  out_u8: 4-byte aligned with 3 channels, 16-byte with 4.  out_hwc4: 16-byte aligned. */
typedef struct TexGSPresent {
    const float* src;           /* [channels, H, W] */
    const float* alpha;         /* [H, W], or NULL */
    const float* background;    /* 3 floats on the device, or NULL for 0, 0, 0 */
    uint8_t* out_u8;
    float* out_hwc4;
    float* out_chw;
    int32_t height;
    int32_t width;
    int32_t channels;           /* 1 or 3 */
    int32_t u8_channels;        /* 3 or 4; read only with out_u8 */
    uint32_t flags;             /* TEXGS_PRESENT_* */
} TexGSPresent;

/* texgs_depth_colour: lo = min, hi = max of depth[p] over the pixels with mask[p] != 0 (all pixels without a mask), then
 *     v   = (depth[p] - lo) / ((hi - lo) + 1e-8f)
 *     v   = min(max(v, 0), 1)
 *     idx = rint(|v * 255.0f|)                   half to even (cvRound), saturated to 0..255, NaN gives 0
 *     rgb = lut[idx], and 0, 0, 0 where mask[p] == 0
 * Outputs, any non-empty subset: out_u8 as above (TEXGS_PRESENT_SWAP_RB is the only flag read), out_hwc4 = rgb / 255.0f and 1.0f,
 * out_chw = rgb / 255.0f; same alignments.  range, when given, receives lo and hi.  Under an all-zero mask every pixel is 0 and range
 * holds +inf, -inf.  The depth under the mask must be finite: that is the caller's guarantee.  Two launches: per-workgroup partial
 * ranges into temp, then the colouring pass, every workgroup of which reduces the partials again. */
typedef struct TexGSDepthColour {
    const float* depth;         /* [H, W] */
    const float* mask;          /* [H, W], or NULL */
    const uint8_t* lut;         /* [256, 3] r, g, b */
    float* range;               /* 2 floats, or NULL */
    uint8_t* out_u8;
    float* out_hwc4;
    float* out_chw;
    int32_t height;
    int32_t width;
    int32_t u8_channels;
    uint32_t flags;
} TexGSDepthColour;

/* texgs_cube_cross: the SH-DC cubemap texture f32 [6, res, res, 3] as an 8-bit horizontal cross [3 res, 4 res, 3]:
 *     v = min(max((x * 0.28209479177387814f) + 0.5f, 0), 1);  byte = (uint8_t) trunc(v * 255.0f), NaN gives 0
 * cell (row, column) of the 3 x 4 grid of res x res cells: (0,1) face 2, (1,0) face 1, (1,1) face 4, (1,2) face 0, (1,3) face 5,
 * (2,1) face 3; the other six cells are written as 0 by the same launch.  1 <= res <= 7168; both pointers 4-byte aligned. */
typedef struct TexGSCubeCross {
    const float* texture;
    uint8_t* out;
    int32_t res;
} TexGSCubeCross;

/* Bytes of `temp` (4-byte aligned) for texgs_depth_colour; 0 for an image it refuses. */
size_t texgs_depth_colour_temp_bytes(int32_t height, int32_t width);

int texgs_present(const TexGSPresent* p, void* stream);
int texgs_depth_colour(const TexGSDepthColour* d, void* temp, size_t temp_bytes, void* stream);
int texgs_cube_cross(const TexGSCubeCross* c, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_PRESENT_H */
