// The row arithmetic of the parameter stage (include/texgs_params.h states it; tests/params_ref.py states it again in numpy), kept
// apart from the kernels so that the same text compiles for the host: tests/test_params_host.py builds it with g++ and compares it
// bit for bit with the numpy statement, on a machine without a GPU.  Every operation is written out in the order of the statement;
// the unit is built with -ffp-contract=off, so none of them is fused.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PM_FN __host__ __device__ __forceinline__
#else
#define PM_FN inline
#endif

namespace params_math {

constexpr float NORM_EPS = 1e-12f;      // F.normalize's eps

// exp after Cephes expf: Cody-Waite reduction by ln 2 in two pieces, degree-5 polynomial, one ldexp
PM_FN float exp32(float x) {
    if (x != x) return x;
    const float xc = x < -110.0f ? -110.0f : (x > 90.0f ? 90.0f : x);
    const float k = rintf(xc * 1.44269504f);
    const float r = (xc - k * 0.693359375f) - k * -2.12194440e-4f;
    float p = 1.9875691500e-4f * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    return ldexpf((p * (r * r) + r) + 1.0f, (int)k);
}

// log of a positive finite number after Cephes logf
PM_FN float log32(float v) {
    int e;
    float m = frexpf(v, &e);
    if (m < 0.707106781186547524f) { e -= 1; m = (m + m) - 1.0f; } else { m = m - 1.0f; }
    const float z = m * m;
    float y = 7.0376836292e-2f * m + -1.1514610310e-1f;
    y = y * m + 1.1676998740e-1f;
    y = y * m + -1.2420140846e-1f;
    y = y * m + 1.4249322787e-1f;
    y = y * m + -1.6668057665e-1f;
    y = y * m + 2.0000714765e-1f;
    y = y * m + -2.4999993993e-1f;
    y = y * m + 3.3333331174e-1f;
    y = (y * m) * z;
    const float fe = (float)e;
    y = y + -2.12194440e-4f * fe;
    y = y - 0.5f * z;
    return (m + y) + 0.693359375f * fe;
}

PM_FN float sigmoid32(float x) { return 1.0f / (1.0f + exp32(-x)); }

PM_FN float norm4(const float q[4]) { return sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }

// F.normalize: q / max(|q|, eps); the max written as a select, so that a NaN norm stays a NaN
PM_FN void normalize(const float q[4], float r[4]) {
    const float n = norm4(q);
    const float d = n < NORM_EPS ? NORM_EPS : n;
    for (int k = 0; k < 4; ++k) r[k] = q[k] / d;
}

PM_FN void normalize_backward(const float q[4], const float g[4], float dq[4]) {
    const float n = norm4(q);
    if (n >= NORM_EPS) {
        float r[4];
        for (int k = 0; k < 4; ++k) r[k] = q[k] / n;
        const float t = ((r[0] * g[0] + r[1] * g[1]) + r[2] * g[2]) + r[3] * g[3];
        for (int k = 0; k < 4; ++k) dq[k] = (g[k] - r[k] * t) / n;
    } else {            // below the clamp the divisor is a constant (a NaN norm lands here too, as with clamp_min's mask)
        for (int k = 0; k < 4; ++k) dq[k] = g[k] / NORM_EPS;
    }
}

PM_FN float clamp_opacity(float o, float eps, float hi) { return o < eps ? eps : (o > hi ? hi : o); }

// one row's term of zero_one_loss
PM_FN float reg_term(float o, float eps) {
    const float v = clamp_opacity(o, eps, 1.0f - eps);
    return log32(v) + log32(1.0f - v);
}

// c = *g_reg / (float) n, or has_reg false
PM_FN float opacity_backward(float o, float g_o, bool has_reg, float c, float eps) {
    float t = 0.0f;
    if (has_reg) {
        const float hi = 1.0f - eps;
        const float v = clamp_opacity(o, eps, hi);
        const float w = 1.0f / v - 1.0f / (1.0f - v);
        t = (eps <= o && o <= hi) ? c * w : 0.0f;
    }
    return (g_o + t) * (o * (1.0f - o));
}

struct Frame3 {          // what the covariance and its backward share: s = m exp(a), q / |q|, R, L = R diag(s)
    float s[3], qh[4], n, R[3][3], L[3][3];
};

PM_FN void frame3(const float a[3], const float q[4], float m, Frame3& f) {
    for (int k = 0; k < 3; ++k) f.s[k] = m * exp32(a[k]);
    f.n = norm4(q);
    for (int k = 0; k < 4; ++k) f.qh[k] = q[k] / f.n;
    const float r = f.qh[0], x = f.qh[1], y = f.qh[2], z = f.qh[3];
    f.R[0][0] = 1.0f - 2.0f * (y * y + z * z);
    f.R[0][1] = 2.0f * (x * y - r * z);
    f.R[0][2] = 2.0f * (x * z + r * y);
    f.R[1][0] = 2.0f * (x * y + r * z);
    f.R[1][1] = 1.0f - 2.0f * (x * x + z * z);
    f.R[1][2] = 2.0f * (y * z - r * x);
    f.R[2][0] = 2.0f * (x * z - r * y);
    f.R[2][1] = 2.0f * (y * z + r * x);
    f.R[2][2] = 1.0f - 2.0f * (x * x + y * y);
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) f.L[i][k] = f.R[i][k] * f.s[k];
}

PM_FN float dot3(const float u[3], const float v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

PM_FN void covariance(const float a[3], const float q[4], float m, float cov[6]) {
    Frame3 f;
    frame3(a, q, m, f);
    cov[0] = dot3(f.L[0], f.L[0]);
    cov[1] = dot3(f.L[0], f.L[1]);
    cov[2] = dot3(f.L[0], f.L[2]);
    cov[3] = dot3(f.L[1], f.L[1]);
    cov[4] = dot3(f.L[1], f.L[2]);
    cov[5] = dot3(f.L[2], f.L[2]);
}

PM_FN void covariance_backward(const float a[3], const float q[4], float m, const float g[6], float da[3], float dq[4]) {
    Frame3 f;
    frame3(a, q, m, f);
    const float M[3][3] = {{2.0f * g[0], g[1], g[2]}, {g[1], 2.0f * g[3], g[4]}, {g[2], g[4], 2.0f * g[5]}};
    float D[3][3];
    for (int k = 0; k < 3; ++k) {
        float dL[3];
        for (int i = 0; i < 3; ++i) dL[i] = (M[i][0] * f.L[0][k] + M[i][1] * f.L[1][k]) + M[i][2] * f.L[2][k];
        da[k] = ((dL[0] * f.R[0][k] + dL[1] * f.R[1][k]) + dL[2] * f.R[2][k]) * f.s[k];
        for (int i = 0; i < 3; ++i) D[i][k] = dL[i] * f.s[k];
    }
    const float r = f.qh[0], x = f.qh[1], y = f.qh[2], z = f.qh[3];
    const float x2 = 2.0f * x, y2 = 2.0f * y, z2 = 2.0f * z;
    float u[4];
    u[0] = 2.0f * ((((((-z) * D[0][1] + y * D[0][2]) + z * D[1][0]) - x * D[1][2]) - y * D[2][0]) + x * D[2][1]);
    u[1] = 2.0f * (((((((y * D[0][1] + z * D[0][2]) + y * D[1][0]) - x2 * D[1][1]) - r * D[1][2]) + z * D[2][0]) + r * D[2][1]) - x2 * D[2][2]);
    u[2] = 2.0f * ((((((((-y2) * D[0][0] + x * D[0][1]) + r * D[0][2]) + x * D[1][0]) + z * D[1][2]) - r * D[2][0]) + z * D[2][1]) - y2 * D[2][2]);
    u[3] = 2.0f * ((((((((-z2) * D[0][0] - r * D[0][1]) + x * D[0][2]) + r * D[1][0]) - z2 * D[1][1]) + y * D[1][2]) + x * D[2][0]) + y * D[2][1]);
    const float t = ((f.qh[0] * u[0] + f.qh[1] * u[1]) + f.qh[2] * u[2]) + f.qh[3] * u[3];
    for (int k = 0; k < 4; ++k) dq[k] = (u[k] - f.qh[k] * t) / f.n;
}

}  // namespace params_math
