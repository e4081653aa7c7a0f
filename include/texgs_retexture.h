/*
 * texgs_retexture.h -- the retexture stage of libtexgs.so (csrc/retexture.hip): the one step of retexture.py that puts a picture INTO
 * the texture (retexture.py:48-58 with TextureGaussian3D.change_texture, models/texture_gaussian3d.py:463-495), from either picture a
 * user paints on -- the 8-bit cubemap cross, or the lat-long map (the inverse of sphere_map, after latlong_to_cubemap of
 * models/modules/NVDIFFREC/util.py:103-117) -- each as ONE streaming pass over the texture.  Additive to the C ABI of texgs.h
 * (TEXGS_ABI_VERSION is unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the launch, so a refused
 * call has changed nothing.  No atomics, no LDS, no host wait, no readback, no allocation: two calls give the same bits.
 *
 * Both entry points end in the same per-texel arithmetic, in fp32 with every operation rounded once (no fused multiply-add, IEEE
 * division); tests/retexture_ref.py states it in numpy.  With C0 = 0.28209479177387814f, old_tex's texel x (3 channels) and the
 * picture's value n (3 channels, in [0, 1]):
 *     o = min(max((C0 * x) + 0.5f, 0), 1)                                  a NaN stays NaN (torch.clamp); not read with mode -1
 *     mode -1   v = n
 *     mode  0   v = n * (((c[0] + c[1]) + c[2]) / 3.0f),  c = min(max(3.0f * o, 0), 1)
 *     mode  1   v = n * o
 *     mode  2   v = o / n                                                   Inf and NaN as IEEE gives them
 *     mode  3   v = n + (((n[0] + n[1]) + n[2]) > 0.01f ? (2.0f * (((o[0] + o[1]) + o[2]) / 3.0f)) * n : o)
 *     out_tex   = (v - 0.5f) / C0
 * out_tex may EQUAL old_tex (in place): a texel reads only its own old texel, and reads it before it is written.  Any other overlap
 * of the two, or of either with src, is refused.  old_tex may be NULL with mode -1, which does not read it; with any other mode a
 * NULL old_tex is refused by name.  old_tex, out_tex and a float src: 4-byte aligned.  Offsets are 64-bit (6 R^2 12 bytes passes
 * 2^31 above R = 5461).
 */
#ifndef TEXGS_RETEXTURE_H
#define TEXGS_RETEXTURE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_RETEX_TEXELS_PER_THREAD 1     /* cross: one texel, 12 bytes, per lane (4 per lane as 16-byte accesses measured slower) */
#define TEXGS_RETEX_THREADS 256             /* threads per workgroup, both kernels */
#define TEXGS_RETEX_MAX_RES 7168            /* the texture limit of texgs.h and texgs_cube_cross */
#define TEXGS_RETEX_MAX_SRC 16384           /* the largest r of a cross and the largest h, w of a lat-long picture */

#define TEXGS_RETEX_RGB 0                   /* src channels are r, g, b */
#define TEXGS_RETEX_BGR 1                   /* src channels are b, g, r, as cv2.imread returns them */

/* texgs_retexture_cross: n of the texel (face f, y, x) is the byte that texture_io.resize_bilinear_u8 gives at cross position
 * (rb R + y, cb R + x) when it resizes the WHOLE cross [3r, 4r] to [3R, 4R], over 255.0f; (rb, cb) of the faces +x, -x, +y, -y, +z, -z:
 * (1,2) (1,0) (0,1) (2,1) (1,1) (1,3).  Per axis, in fp64 (n_in = 3r or 4r, n_out = 3R or 4R, o the output index):
 *     s = ((o + 0.5) * (n_in / n_out)) - 0.5;  i0 = floor(s);  w = s - i0;  i1 = min(max(i0 + 1, 0), n_in - 1);
 *     w = i0 < 0 ? 0 : w;  i0 = min(max(i0, 0), n_in - 1)
 * so a tap near a cell border reads the neighbouring cell, an unused one included, and clamping is at the cross's edge only.  Per
 * channel, in fp64:
 *     top = (a[y0][x0] * (1 - wx)) + (a[y0][x1] * wx);  bot = (a[y1][x0] * (1 - wx)) + (a[y1][x1] * wx)
 *     byte = min(max(floor(((top * (1 - wy)) + (bot * wy)) + 0.5), 0), 255)
 * Only the source pixels under the taps of the six used cells are read; r = R is no special case (the weights are exactly 0). */
typedef struct TexGSRetexCross {
    const uint8_t* src;         /* [3r, 4r, 3] */
    const float* old_tex;       /* [6, R, R, 3], or NULL with mode -1 */
    float* out_tex;             /* [6, R, R, 3]; may equal old_tex */
    int32_t r;                  /* 1 .. TEXGS_RETEX_MAX_SRC */
    int32_t R;                  /* 1 .. TEXGS_RETEX_MAX_RES */
    int32_t mode;               /* -1, 0, 1, 2, 3 */
    int32_t order;              /* TEXGS_RETEX_RGB or TEXGS_RETEX_BGR */
} TexGSRetexCross;

/* texgs_retexture_latlong: latlong_to_cubemap, then the arithmetic above.  For the texel (face s, row i, column j), in fp64:
 *     gx = (2j + 1) / R - 1;  gy = (2i + 1) / R - 1
 *     d  = (1, -gy, -gx) (-1, -gy, gx) (gx, 1, gy) (gx, -1, -gy) (gx, -gy, 1) (-gx, -gy, -1) for s = 0..5;  v = d / |d|
 *     tu = atan2(v[0], -v[2]) / (2 pi) + 0.5;  tv = acos(min(max(v[1], -1), 1)) / pi
 *     px = tu w - 0.5;  x0 = floor(px);  wx = px - x0;  x1 = x0 + 1;  x0, x1 taken modulo w      (and the same with tv, h)
 * BOTH axes wrap (nvdiffrast's default boundary mode of a 2-D texture).  wx and wy are rounded to fp32 once; then in fp32
 *     top = (a[y0][x0] * (1 - wx)) + (a[y0][x1] * wx);  bot likewise with y1;  n = (top * (1 - wy)) + (bot * wy)
 * with a = src, or src / 255.0f for bytes.  These conventions are restated from the reference's source and are UNPINNED against
 * nvdiffrast, which has no ROCm build to compare with. */
typedef struct TexGSRetexLatLong {
    const void* src;            /* [h, w, 3], float or uint8_t */
    const float* old_tex;       /* [6, R, R, 3], or NULL with mode -1 */
    float* out_tex;             /* [6, R, R, 3]; may equal old_tex */
    int32_t h;                  /* 1 .. TEXGS_RETEX_MAX_SRC */
    int32_t w;                  /* 1 .. TEXGS_RETEX_MAX_SRC */
    int32_t R;                  /* 1 .. TEXGS_RETEX_MAX_RES */
    int32_t mode;               /* -1, 0, 1, 2, 3 */
    int32_t src_u8;             /* 0: src is float, 1: src is uint8_t and a value is v / 255.0f */
} TexGSRetexLatLong;

int texgs_retexture_cross(const TexGSRetexCross* c, void* stream);
int texgs_retexture_latlong(const TexGSRetexLatLong* l, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_RETEXTURE_H */
