/*
 * texgs_params.h -- the parameter stage of libtexgs.so (csrc/params.hip): what the reference's getters do to the stored parameters
 * before every render (models/texture_gaussian3d.py: get_scaling = exp, get_rotation = F.normalize, get_opacity = sigmoid), the
 * opacity regulariser on top of them (losses/zero_one_loss.py, `lambda_opacity_reg`) and get_covariance (utils/general.py:
 * build_rotation, build_scaling_rotation, strip_lowerdiag), each with its backward.  Additive to the C ABI of texgs.h
 * (TEXGS_ABI_VERSION is unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.  No atomics, no host wait, no readback: two calls give the same bits.  All pointers 4-byte
 * aligned; rotation, rotations, g_rotations and d_rotation 16-byte aligned (a quaternion moves as one 16-byte access); temp 8-byte
 * aligned.  n = 0 launches nothing and accepts NULL pointers everywhere, except that `reg` with n = 0 is refused (a mean over nothing).
 *
 * The arithmetic is a bit-exact contract, float32 unless said otherwise, every operation rounded once, no fused multiply-add, IEEE
 * division and square root, subnormals kept.  tests/params_ref.py states it in numpy with the same operation order, exp and log
 * included: they are the two polynomials below, not a math library's, so that a row's bits depend on the row alone -- not on n, on
 * the row's position, or on the library version.
 *
 *     exp(x):  x NaN -> NaN.  x' = x < -110 ? -110 : (x > 90 ? 90 : x);  k = rint(x' * 1.44269504f)  (ties to even)
 *              r = (x' - k * 0.693359375f) - k * -2.12194440e-4f
 *              p = ((((1.9875691500e-4f r + 1.3981999507e-3f) r + 8.3334519073e-3f) r + 4.1665795894e-2f) r + 1.6666665459e-1f) r
 *                  + 5.0000001201e-1f
 *              exp = ldexp((p * (r * r) + r) + 1.0f, k)         (one rounding, also into the subnormals; above the range: +inf)
 *     log(v):  v a positive finite number.  (m, e) = frexp(v);  if m < 0.707106781186547524f: e = e - 1, m = (m + m) - 1.0f
 *              else m = m - 1.0f.  z = m * m;  with the nine coefficients c0 .. c8 = 7.0376836292e-2f, -1.1514610310e-1f,
 *              1.1676998740e-1f, -1.2420140846e-1f, 1.4249322787e-1f, -1.6668057665e-1f, 2.0000714765e-1f, -2.4999993993e-1f,
 *              3.3333331174e-1f:   y = ((((((((c0 m + c1) m + c2) m + c3) m + c4) m + c5) m + c6) m + c7) m + c8) m * z
 *              y = y + -2.12194440e-4f * (float) e;  y = y - 0.5f * z;  log = (m + y) + 0.693359375f * (float) e
 * (both after the Cephes single-precision routines; within one unit in the last place of the exact value: measured 0.96 for exp over
 * [-104, 88] and 0.77 for log over the positive normal numbers, tests/test_params_host.py.)
 */
#ifndef TEXGS_PARAMS_H
#define TEXGS_PARAMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_PARAMS_ROWS_PER_WORKGROUP 256     /* one thread per row; the rows one fp64 partial of the regulariser covers */

/* texgs_params_activate.  Per row i (a = scaling, q = rotation, x = opacity):
 *     scales[i][k]  = exp(a[k])                                                          k = 0, 1, 2
 *     n = sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3);  rotations[i][k] = q[k] / max(n, 1e-12f)        (F.normalize)
 *     opacities[i]  = o = 1.0f / (1.0f + exp(-x))
 * (max and min are selects: max(n, e) = n < e ? e : n, so a NaN stays a NaN.)  A square that overflows gives n = inf and the row 0
 * (or NaN where a component is inf); squares that underflow give n = 0 and the row q / 1e-12f.  This is the float32 statement,
 * whatever another library does there.
 * With reg:   hi = 1.0f - epsilon;  v = min(max(o, epsilon), hi);  term = log(v) + log(1.0f - v)       (float32)
 *             *reg = (float) (sum_i (double) term_i / (double) n)
 * the sum in fp64 in a fixed order (within a workgroup: a tree over its 256 rows; then partial j, j + 256, ... by thread j of ONE
 * workgroup and the same tree), rounded to float32 once.  One launch; with reg a second launch of one workgroup.
 * An output pointer that is NULL is not computed, and its input is then not read and may be NULL; not all of scales, rotations,
 * opacities and reg may be NULL.  reg needs temp of texgs_params_temp_bytes(n) bytes; without reg temp is not read. */
typedef struct TexGSParamsActivate {
    const float* scaling;       /* [n, 3], read for scales */
    const float* rotation;      /* [n, 4], read for rotations */
    const float* opacity;       /* [n], read for opacities and reg */
    float* scales;              /* [n, 3], or NULL */
    float* rotations;           /* [n, 4], or NULL */
    float* opacities;           /* [n], or NULL */
    float* reg;                 /* one float on the device, or NULL */
    float epsilon;              /* read with reg only: in (0, 0.5) */
    int32_t n;
} TexGSParamsActivate;

/* texgs_params_activate_backward.  Upstream gradients g_*: a NULL pointer is a zero gradient.  Per row, with s = scales and
 * o = opacities as the forward left them and q the raw rotation:
 *     d_scaling[k] = g_scales[k] * s[k]
 *     n, d = max(n, 1e-12f) and r = q / d as in the forward;  t = ((r0 g0 + r1 g1) + r2 g2) + r3 g3      (g = g_rotations)
 *     d_rotation[k] = n >= 1e-12f ? (g[k] - r[k] * t) / n : g[k] / 1e-12f              (what autograd gives through clamp_min)
 *     c = *g_reg / (float) n_rows;  hi, v as in the forward;  w = 1.0f / v - 1.0f / (1.0f - v)
 *     d_opacity = (g_opacities + ((epsilon <= o && o <= hi) ? c * w : 0.0f)) * (o * (1.0f - o))
 * (the term in c is absent when g_reg is NULL).  d_* that is NULL is not computed, and a d_* whose upstream gradients are all NULL
 * is written as zeros; what such an output alone needs is not read and may be NULL: scales for d_scaling, rotation for d_rotation,
 * opacities for d_opacity.  Not all of d_scaling, d_rotation and d_opacity may be NULL.  Written, not accumulated.  One launch. */
typedef struct TexGSParamsActivateGrad {
    const float* scales;        /* [n, 3], the forward's output */
    const float* rotation;      /* [n, 4], the raw parameter */
    const float* opacities;     /* [n], the forward's output */
    const float* g_scales;      /* [n, 3], or NULL */
    const float* g_rotations;   /* [n, 4], or NULL */
    const float* g_opacities;   /* [n], or NULL */
    const float* g_reg;         /* one float on the device, or NULL */
    float* d_scaling;           /* [n, 3], or NULL */
    float* d_rotation;          /* [n, 4], or NULL */
    float* d_opacity;           /* [n], or NULL */
    float epsilon;              /* read with g_reg only: in (0, 0.5) */
    int32_t n;
} TexGSParamsActivateGrad;

/* texgs_params_covariance: get_covariance.  Per row, m = scale_modifier:
 *     s[k] = m * exp(a[k]);  n as above;  (r, x, y, z) = q / n          (no epsilon, as build_rotation has it: a zero quaternion
 *                                                                         gives a non-finite row; documented, not checked)
 *     R00 = 1.0f - 2.0f (y y + z z)   R01 = 2.0f (x y - r z)          R02 = 2.0f (x z + r y)
 *     R10 = 2.0f (x y + r z)          R11 = 1.0f - 2.0f (x x + z z)   R12 = 2.0f (y z - r x)
 *     R20 = 2.0f (x z - r y)          R21 = 2.0f (y z + r x)          R22 = 1.0f - 2.0f (x x + y y)
 *     L[i][k] = R[i][k] * s[k];  S[i][j] = (L[i][0] L[j][0] + L[i][1] L[j][1]) + L[i][2] L[j][2]
 *     cov = (S00, S01, S02, S11, S12, S22)                                                 (the order of strip_lowerdiag)
 * One launch. */
typedef struct TexGSParamsCovariance {
    const float* scaling;       /* [n, 3] */
    const float* rotation;      /* [n, 4] */
    float* cov;                 /* [n, 6] */
    float scale_modifier;       /* finite and positive */
    int32_t n;
} TexGSParamsCovariance;

/* texgs_params_covariance_backward.  g = g_cov; s, n, (r, x, y, z), R and L are recomputed as above.
 *     M = [[2 g0, g1, g2], [g1, 2 g3, g4], [g2, g4, 2 g5]];  dL[i][k] = (M[i][0] L[0][k] + M[i][1] L[1][k]) + M[i][2] L[2][k]
 *     d_scaling[k] = ((dL[0][k] R[0][k] + dL[1][k] R[1][k]) + dL[2][k] R[2][k]) * s[k];   D[i][k] = dL[i][k] * s[k]
 *     dr = 2 ((((((-z) D01 + y D02) + z D10) - x D12) - y D20) + x D21)
 *     dx = 2 ((((((((y D01 + z D02) + y D10) - (2 x) D11) - r D12) + z D20) + r D21) - (2 x) D22)
 *     dy = 2 (((((((((-(2 y)) D00 + x D01) + r D02) + x D10) + z D12) - r D20) + z D21) - (2 y) D22)
 *     dz = 2 (((((((((-(2 z)) D00 - r D01) + x D02) + r D10) - (2 z) D11) + y D12) + x D20) + y D21)
 *     u = (dr, dx, dy, dz), qh = (r, x, y, z);  t = ((qh0 u0 + qh1 u1) + qh2 u2) + qh3 u3;  d_rotation[k] = (u[k] - qh[k] * t) / n
 * g_cov NULL is a zero gradient; d_scaling or d_rotation may be NULL, not both.  Written, not accumulated.  One launch. */
typedef struct TexGSParamsCovarianceGrad {
    const float* scaling;       /* [n, 3] */
    const float* rotation;      /* [n, 4] */
    const float* g_cov;         /* [n, 6], or NULL */
    float* d_scaling;           /* [n, 3], or NULL */
    float* d_rotation;          /* [n, 4], or NULL */
    float scale_modifier;
    int32_t n;
} TexGSParamsCovarianceGrad;

/* Bytes of `temp` (8-byte aligned) for texgs_params_activate with reg: one double per workgroup; 0 for n <= 0. */
size_t texgs_params_temp_bytes(int32_t n);

int texgs_params_activate(const TexGSParamsActivate* a, void* temp, size_t temp_bytes, void* stream);
int texgs_params_activate_backward(const TexGSParamsActivateGrad* g, void* stream);
int texgs_params_covariance(const TexGSParamsCovariance* c, void* stream);
int texgs_params_covariance_backward(const TexGSParamsCovarianceGrad* g, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_PARAMS_H */
