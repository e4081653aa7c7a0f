// The per-row arithmetic of the colour stage (include/texgs_shcolor.h states it; tests/shcolor_ref.py states it again in numpy), kept
// apart from the kernels so that the same text compiles for the host: tests/test_shcolor_host.py builds it with g++ and compares it
// bit for bit with the numpy statement, on a machine without a GPU.  Every operation is written out with the parentheses of the
// statement; the unit is built with -ffp-contract=off, so none of them is fused.  The degree is a template argument: every index
// below is a constant after unrolling, so the basis and the gradient row live in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SM_FN __host__ __device__ __forceinline__
#else
#define SM_FN inline
#endif

namespace shcolor_math {

constexpr int coeffs_of(int deg) { return (deg + 1) * (deg + 1); }

// the real SH constants (utils/sh.py), rounded to float32 once
constexpr float c0 = 0.28209479177387814f;
constexpr float c1 = 0.4886025119029199f;
constexpr float c2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
constexpr float c3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f,
                         1.445305721320277f, -0.5900435899266435f};
constexpr float c4[9] = {2.5033429417967046f, -1.7701307697799304f, 0.9461746957575601f, -0.6690465435572892f, 0.10578554691520431f,
                         -0.6690465435572892f, 0.47308734787878004f, -1.7701307697799304f, 0.6258357354491761f};

// p = xyz - campos, n = |p|, d = p / n as three divisions; p == 0 gives 0 / 0, as the reference does
SM_FN float direction(const float xyz[3], const float cam[3], float d[3]) {
    const float px = xyz[0] - cam[0], py = xyz[1] - cam[1], pz = xyz[2] - cam[2];
    const float n = sqrtf((px * px + py * py) + pz * pz);
    d[0] = px / n; d[1] = py / n; d[2] = pz / n;
    return n;
}

// the signed basis: b[k] * sh[k] are the terms of the reference's eval_sh, each product chain left to right
template <int DEG>
SM_FN void basis(float x, float y, float z, float* b) {
    b[0] = c0;
    if constexpr (DEG >= 1) {
        b[1] = -(c1 * y);
        b[2] = c1 * z;
        b[3] = -(c1 * x);
    }
    if constexpr (DEG >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        const float xy = x * y, yz = y * z, xz = x * z;
        b[4] = c2[0] * xy;
        b[5] = c2[1] * yz;
        b[6] = c2[2] * (((2.0f * zz) - xx) - yy);
        b[7] = c2[3] * xz;
        b[8] = c2[4] * (xx - yy);
        if constexpr (DEG >= 3) {
            b[9] = (c3[0] * y) * ((3.0f * xx) - yy);
            b[10] = (c3[1] * xy) * z;
            b[11] = (c3[2] * y) * (((4.0f * zz) - xx) - yy);
            b[12] = (c3[3] * z) * (((2.0f * zz) - (3.0f * xx)) - (3.0f * yy));
            b[13] = (c3[4] * x) * (((4.0f * zz) - xx) - yy);
            b[14] = (c3[5] * z) * (xx - yy);
            b[15] = (c3[6] * x) * (xx - (3.0f * yy));
        }
        if constexpr (DEG >= 4) {
            b[16] = (c4[0] * xy) * (xx - yy);
            b[17] = (c4[1] * yz) * ((3.0f * xx) - yy);
            b[18] = (c4[2] * xy) * ((7.0f * zz) - 1.0f);
            b[19] = (c4[3] * yz) * ((7.0f * zz) - 3.0f);
            b[20] = c4[4] * ((zz * ((35.0f * zz) - 30.0f)) + 3.0f);
            b[21] = (c4[5] * xz) * ((7.0f * zz) - 3.0f);
            b[22] = (c4[6] * (xx - yy)) * ((7.0f * zz) - 1.0f);
            b[23] = (c4[7] * xz) * (xx - (3.0f * yy));
            b[24] = c4[8] * ((xx * (xx - (3.0f * yy))) - (yy * ((3.0f * xx) - yy)));
        }
    }
}

// dd = sum_k grad b_k * t[k]: the terms that are not identically zero, in the statement's order, each sum starting at zero
template <int DEG>
SM_FN void dir_grad(float x, float y, float z, const float* t, float dd[3]) {
    float ddx = 0.0f, ddy = 0.0f, ddz = 0.0f;
    if constexpr (DEG >= 1) {
        ddy = ddy + (-c1) * t[1];
        ddz = ddz + c1 * t[2];
        ddx = ddx + (-c1) * t[3];
    }
    if constexpr (DEG >= 2) {
        ddx = ddx + (c2[0] * y) * t[4];
        ddy = ddy + (c2[0] * x) * t[4];
        ddy = ddy + (c2[1] * z) * t[5];
        ddz = ddz + (c2[1] * y) * t[5];
        ddx = ddx + (c2[2] * (-2.0f * x)) * t[6];
        ddy = ddy + (c2[2] * (-2.0f * y)) * t[6];
        ddz = ddz + (c2[2] * (4.0f * z)) * t[6];
        ddx = ddx + (c2[3] * z) * t[7];
        ddz = ddz + (c2[3] * x) * t[7];
        ddx = ddx + (c2[4] * (2.0f * x)) * t[8];
        ddy = ddy + (c2[4] * (-2.0f * y)) * t[8];
    }
    if constexpr (DEG >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z;
        const float xy = x * y, yz = y * z, xz = x * z;
        ddx = ddx + (c3[0] * (6.0f * xy)) * t[9];
        ddy = ddy + (c3[0] * ((3.0f * xx) - (3.0f * yy))) * t[9];
        ddx = ddx + (c3[1] * yz) * t[10];
        ddy = ddy + (c3[1] * xz) * t[10];
        ddz = ddz + (c3[1] * xy) * t[10];
        ddx = ddx + (c3[2] * (-2.0f * xy)) * t[11];
        ddy = ddy + (c3[2] * (((4.0f * zz) - xx) - (3.0f * yy))) * t[11];
        ddz = ddz + (c3[2] * (8.0f * yz)) * t[11];
        ddx = ddx + (c3[3] * (-6.0f * xz)) * t[12];
        ddy = ddy + (c3[3] * (-6.0f * yz)) * t[12];
        ddz = ddz + (c3[3] * (((6.0f * zz) - (3.0f * xx)) - (3.0f * yy))) * t[12];
        ddx = ddx + (c3[4] * (((4.0f * zz) - (3.0f * xx)) - yy)) * t[13];
        ddy = ddy + (c3[4] * (-2.0f * xy)) * t[13];
        ddz = ddz + (c3[4] * (8.0f * xz)) * t[13];
        ddx = ddx + (c3[5] * (2.0f * xz)) * t[14];
        ddy = ddy + (c3[5] * (-2.0f * yz)) * t[14];
        ddz = ddz + (c3[5] * (xx - yy)) * t[14];
        ddx = ddx + (c3[6] * ((3.0f * xx) - (3.0f * yy))) * t[15];
        ddy = ddy + (c3[6] * (-6.0f * xy)) * t[15];
        if constexpr (DEG >= 4) {
            const float xyz = xy * z;
            ddx = ddx + ((c4[0] * y) * ((3.0f * xx) - yy)) * t[16];
            ddy = ddy + ((c4[0] * x) * (xx - (3.0f * yy))) * t[16];
            ddx = ddx + (c4[1] * (6.0f * xyz)) * t[17];
            ddy = ddy + ((c4[1] * z) * ((3.0f * xx) - (3.0f * yy))) * t[17];
            ddz = ddz + ((c4[1] * y) * ((3.0f * xx) - yy)) * t[17];
            ddx = ddx + ((c4[2] * y) * ((7.0f * zz) - 1.0f)) * t[18];
            ddy = ddy + ((c4[2] * x) * ((7.0f * zz) - 1.0f)) * t[18];
            ddz = ddz + (c4[2] * (14.0f * xyz)) * t[18];
            ddy = ddy + ((c4[3] * z) * ((7.0f * zz) - 3.0f)) * t[19];
            ddz = ddz + ((c4[3] * y) * ((21.0f * zz) - 3.0f)) * t[19];
            ddz = ddz + ((c4[4] * z) * ((140.0f * zz) - 60.0f)) * t[20];
            ddx = ddx + ((c4[5] * z) * ((7.0f * zz) - 3.0f)) * t[21];
            ddz = ddz + ((c4[5] * x) * ((21.0f * zz) - 3.0f)) * t[21];
            ddx = ddx + ((c4[6] * (2.0f * x)) * ((7.0f * zz) - 1.0f)) * t[22];
            ddy = ddy + ((c4[6] * (-2.0f * y)) * ((7.0f * zz) - 1.0f)) * t[22];
            ddz = ddz + ((c4[6] * (xx - yy)) * (14.0f * z)) * t[22];
            ddx = ddx + ((c4[7] * z) * ((3.0f * xx) - (3.0f * yy))) * t[23];
            ddy = ddy + (c4[7] * (-6.0f * xyz)) * t[23];
            ddz = ddz + ((c4[7] * x) * (xx - (3.0f * yy))) * t[23];
            ddx = ddx + ((c4[8] * (4.0f * x)) * (xx - (3.0f * yy))) * t[24];
            ddy = ddy + ((c4[8] * (4.0f * y)) * (yy - (3.0f * xx))) * t[24];
        }
    }
    dd[0] = ddx; dd[1] = ddy; dd[2] = ddz;
}

// v_c = (((b_0 sh[0,c]) + b_1 sh[1,c]) + ...), sh laid out [k][c]
template <int DEG>
SM_FN void eval(const float* b, const float* sh, float v[3]) {
    constexpr int KA = coeffs_of(DEG);
    for (int c = 0; c < 3; ++c) v[c] = b[0] * sh[c];
#pragma unroll
    for (int k = 1; k < KA; ++k)
        for (int c = 0; c < 3; ++c) v[c] = v[c] + b[k] * sh[3 * k + c];
}

// the +0.5 and the clamp as a select: a NaN stays a NaN (fmaxf would swallow it)
SM_FN float clamp_colour(float v) {
    const float w = v + 0.5f;
    return w < 0.0f ? 0.0f : w;
}

// One row of the forward.  sh: the row's coefficients [k][c], the first (DEG + 1)^2 of them.  eval_mode: `xyz` holds the
// direction to use as given, and the value leaves without the +0.5 and the clamp.
template <int DEG>
SM_FN void row_forward(const float* sh, const float xyz[3], const float cam[3], bool eval_mode, float out[3]) {
    float d[3] = {0.0f, 0.0f, 0.0f}, b[coeffs_of(DEG)], v[3];
    if constexpr (DEG >= 1) {
        if (eval_mode) { d[0] = xyz[0]; d[1] = xyz[1]; d[2] = xyz[2]; } else { direction(xyz, cam, d); }
    }
    basis<DEG>(d[0], d[1], d[2], b);
    eval<DEG>(b, sh, v);
    for (int c = 0; c < 3; ++c) out[c] = eval_mode ? v[c] : clamp_colour(v[c]);
}

// One row and one view of the backward: the forward recomputed, then acc_sh[3 k + c] += b_k g_c and acc_xyz += d_xyz of this view
// (in eval_mode: no gate, and acc_xyz += dd).  want_sh / want_xyz: what is not wanted is not computed.
template <int DEG>
SM_FN void row_backward_view(const float* sh, const float xyz[3], const float cam[3], const float upstream[3], bool eval_mode,
                             bool want_sh, bool want_xyz, float* acc_sh, float acc_xyz[3]) {
    constexpr int KA = coeffs_of(DEG);
    float d[3] = {0.0f, 0.0f, 0.0f}, b[KA], v[3], g[3];
    float n = 1.0f;
    if constexpr (DEG >= 1) {
        if (eval_mode) { d[0] = xyz[0]; d[1] = xyz[1]; d[2] = xyz[2]; } else { n = direction(xyz, cam, d); }
    }
    basis<DEG>(d[0], d[1], d[2], b);
    if (eval_mode) {
        for (int c = 0; c < 3; ++c) g[c] = upstream[c];
    } else {
        eval<DEG>(b, sh, v);
        for (int c = 0; c < 3; ++c) g[c] = (v[c] + 0.5f >= 0.0f) ? upstream[c] : 0.0f;      // clamp_min passes the gradient at equality
    }
    if (want_sh) {
#pragma unroll
        for (int k = 0; k < KA; ++k)
            for (int c = 0; c < 3; ++c) acc_sh[3 * k + c] = acc_sh[3 * k + c] + b[k] * g[c];
    }
    if constexpr (DEG >= 1) {
        if (want_xyz) {
            float t[KA], dd[3];
            t[0] = 0.0f;
#pragma unroll
            for (int k = 1; k < KA; ++k) t[k] = ((g[0] * sh[3 * k]) + (g[1] * sh[3 * k + 1])) + (g[2] * sh[3 * k + 2]);
            dir_grad<DEG>(d[0], d[1], d[2], t, dd);
            if (eval_mode) {
                for (int i = 0; i < 3; ++i) acc_xyz[i] = acc_xyz[i] + dd[i];
            } else {
                const float dot = ((d[0] * dd[0]) + (d[1] * dd[1])) + (d[2] * dd[2]);
                for (int i = 0; i < 3; ++i) acc_xyz[i] = acc_xyz[i] + (dd[i] - (d[i] * dot)) / n;
            }
        }
    }
}

}  // namespace shcolor_math
