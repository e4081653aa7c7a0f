/*
 * texgs_shcolor.h -- the colour stage of libtexgs.so (csrc/shcolor.hip): spherical harmonics of degree 0..4 in the view direction to
 * a colour per Gaussian, what the reference's render glue does under `convert_SHs_python` (render/render.py:64-68 with
 * utils/sh.py:eval_sh) before it hands `colors_precomp` to the rasterizer, and its backward.  Additive to the C ABI of texgs.h
 * (TEXGS_ABI_VERSION is unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.  No atomics, no host wait, no readback: two calls give the same bits.  All pointers 4-byte
 * aligned.  n = 0 launches nothing.
 *
 * The arithmetic is a bit-exact contract: float32, every operation rounded once, no fused multiply-add, IEEE division and square
 * root.  tests/shcolor_ref.py states it in numpy with the same operation order.  Per Gaussian i and view, with K = coeffs and
 * the active count A = (degree + 1)^2 <= K (only the first A coefficients of a row are read):
 *
 *     p = xyz[i] - campos;   n = sqrt((px px + py py) + pz pz);   d = p / n                      (three divisions, no epsilon)
 *     b_0 .. b_{A-1}: the signed real SH basis in d, every constant rounded to float32 first, (x, y, z) = d, xx = x x, xy = x y ...:
 *       b0 = C0                       b1 = -(C1 y)                     b2 = C1 z                       b3 = -(C1 x)
 *       b4 = C2[0] xy                 b5 = C2[1] yz                    b6 = C2[2] (((2 zz) - xx) - yy)
 *       b7 = C2[3] xz                 b8 = C2[4] (xx - yy)
 *       b9  = (C3[0] y) ((3 xx) - yy)                 b10 = (C3[1] xy) z            b11 = (C3[2] y) (((4 zz) - xx) - yy)
 *       b12 = (C3[3] z) (((2 zz) - (3 xx)) - (3 yy))  b13 = (C3[4] x) (((4 zz) - xx) - yy)
 *       b14 = (C3[5] z) (xx - yy)                     b15 = (C3[6] x) (xx - (3 yy))
 *       b16 = (C4[0] xy) (xx - yy)                    b17 = (C4[1] yz) ((3 xx) - yy)          b18 = (C4[2] xy) ((7 zz) - 1)
 *       b19 = (C4[3] yz) ((7 zz) - 3)                 b20 = C4[4] ((zz ((35 zz) - 30)) + 3)   b21 = (C4[5] xz) ((7 zz) - 3)
 *       b22 = (C4[6] (xx - yy)) ((7 zz) - 1)          b23 = (C4[7] xz) (xx - (3 yy))
 *       b24 = C4[8] ((xx (xx - (3 yy))) - (yy ((3 xx) - yy)))
 *     (C0 .. C4 are the constants of utils/sh.py; the products with sh below complete the reference's terms in its order)
 *     v_c = (((b_0 sh[i,0,c]) + b_1 sh[i,1,c]) + b_2 sh[i,2,c]) + ...                              (left to right)
 *     colour_c = (v_c + 0.5f < 0) ? 0 : v_c + 0.5f                                                (a select: a NaN stays a NaN)
 * A Gaussian at the camera centre gives 0 / 0: at degree >= 1 its colour in that view is NaN, as in the reference.  Degree 0 reads
 * neither xyz nor campos.
 *
 * Backward, the forward recomputed in the same arithmetic; the views of a call in the order given, every sum starting at zero (or,
 * with `accumulate`, at what the outputs hold), each step a rounded product followed by a rounded add:
 *     g_c = (v_c + 0.5f >= 0) ? g_colors[i,c] : 0                                                (clamp_min passes the gradient at equality)
 *     d_sh[i,k,c] = d_sh[i,k,c] + b_k g_c                      k < A;  the coefficients k >= A are written as zeros
 *     t_k = ((g_0 sh[i,k,0]) + (g_1 sh[i,k,1])) + (g_2 sh[i,k,2])                                  1 <= k < A
 *     dd  = sum_k grad b_k t_k: the terms that are not identically zero, in the order and with the parentheses of dir_grad() in
 *           csrc/shcolor_math.h (and of tests/shcolor_ref.py), x, y and z taken as independent, as autograd takes them
 *     dot = ((dx ddx) + (dy ddy)) + (dz ddz);    d_xyz[i,j] = d_xyz[i,j] + (dd_j - (d_j dot)) / n
 * At degree 0 d_xyz is zero.  campos gets no gradient.
 *
 * mode TEXGS_SH_EVAL is the middle alone, the reference's eval_sh: `xyz` holds the directions, used as given; the value leaves
 * without the +0.5 and the clamp; the backward has no gate and d_xyz = 0 + dd.  It takes exactly one view, whose campos is not read.
 */
#ifndef TEXGS_SHCOLOR_H
#define TEXGS_SHCOLOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_SH_COLORS_ROWS_PER_WORKGROUP 128  /* one thread per Gaussian; 128 rows of 75 floats are 38.4 KB of LDS */
#define TEXGS_SH_COLORS_ROWS_PER_WORKGROUP_DEG4 256     /* the degree-4 forward: the row staged in two passes of at most 48 floats */
#define TEXGS_SH_COLORS_MAX_VIEWS 16            /* view records one launch carries by value in its kernel arguments */
#define TEXGS_SH_COLORS_MAX_DEGREE 4

#define TEXGS_SH_COLORS 0       /* mode: direction from xyz and campos, +0.5, clamp at zero */
#define TEXGS_SH_EVAL 1         /* mode: eval_sh on the caller's directions */
#define TEXGS_SH_LAYOUT_KC 0    /* sh is [n, coeffs, 3]: what get_features returns, and what its transpose(1, 2) still is in memory */
#define TEXGS_SH_LAYOUT_CK 1    /* sh is [n, 3, coeffs], contiguous */

/* One view of the forward (16 bytes). */
typedef struct TexGSShColorView {
    const float* campos;        /* f32[3], device; not read in mode TEXGS_SH_EVAL and at degree 0 */
    float* colors;              /* f32[n, 3], device: this view's output */
} TexGSShColorView;

/* One view of the backward (16 bytes). */
typedef struct TexGSShColorGradView {
    const float* campos;        /* f32[3], device */
    const float* g_colors;      /* f32[n, 3], device: the upstream gradient of this view's output */
} TexGSShColorGradView;

/* The coefficients come as one tensor `sh` (layout says which) or as the pair sh_dc [n, 1, 3] and sh_rest [n, coeffs - 1, 3]
 * (sh NULL, layout TEXGS_SH_LAYOUT_KC; sh_rest may be NULL when degree is 0). */
typedef struct TexGSShColors {
    const float* sh;
    const float* sh_dc;
    const float* sh_rest;
    const float* xyz;           /* [n, 3]: the means, or the directions in mode TEXGS_SH_EVAL; may be NULL at degree 0 */
    int32_t n;
    int32_t coeffs;             /* K: 1, 4, 9, 16 or 25 */
    int32_t degree;             /* 0..4, (degree + 1)^2 <= coeffs */
    int32_t layout;
    int32_t mode;
} TexGSShColors;

/* The gradients are written (with accumulate != 0: added to, the outputs' contents being the sums of the views before), in the
 * layout of the input they belong to: d_sh with sh, d_sh_dc and d_sh_rest with the pair.  An output that is NULL is not computed;
 * not all of them may be NULL. */
typedef struct TexGSShColorsGrad {
    const float* sh;
    const float* sh_dc;
    const float* sh_rest;
    const float* xyz;
    float* d_sh;                /* like sh, or NULL */
    float* d_sh_dc;             /* [n, 1, 3], or NULL */
    float* d_sh_rest;           /* [n, coeffs - 1, 3], or NULL */
    float* d_xyz;               /* [n, 3], or NULL */
    int32_t n;
    int32_t coeffs;
    int32_t degree;
    int32_t layout;
    int32_t mode;
    int32_t accumulate;         /* 0 or 1: the second and later calls of a step with more than TEXGS_SH_COLORS_MAX_VIEWS views */
} TexGSShColorsGrad;

/* One launch for `count` views, 1 <= count <= TEXGS_SH_COLORS_MAX_VIEWS: the coefficient rows are read once.  Refused by name:
 * a NULL descriptor or record array, degree outside 0..4, coeffs not in {1, 4, 9, 16, 25}, (degree + 1)^2 > coeffs, n < 0,
 * n * coeffs * 3 >= 2^31, count < 1 or above the maximum (in mode TEXGS_SH_EVAL: count != 1), an unknown layout or mode, the pair
 * with layout TEXGS_SH_LAYOUT_CK, both sh and the pair, and with n > 0 a NULL or misaligned pointer where one is required. */
int texgs_sh_colors_forward(const TexGSShColors* c, const TexGSShColorView* views, int32_t count, void* stream);
/* One launch for `count` views; more views take several calls in view order, the later ones with accumulate = 1. */
int texgs_sh_colors_backward(const TexGSShColorsGrad* g, const TexGSShColorGradView* views, int32_t count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_SHCOLOR_H */
