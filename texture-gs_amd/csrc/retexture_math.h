// The per-texel arithmetic of the retexture stage (include/texgs_retexture.h states it; tests/retexture_ref.py states it again in
// numpy), kept apart from the kernels so that the same text compiles for the host: tests/test_retexture_host.py builds it with g++
// and compares it bit for bit with the numpy statement, on a machine without a GPU.  Every operation is written out in the order of
// the statement; the unit is built with -ffp-contract=off, so none of them is fused.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RM_FN __host__ __device__ __forceinline__
#else
#define RM_FN inline
#endif

namespace retexture_math {

constexpr float C0 = 0.28209479177387814f;

// (row, column) of face f's cell in the 3 x 4 cross, a nibble per face: texture_io._CROSS_POS
RM_FN int cross_row(int f) { return (0x112011 >> (4 * f)) & 15; }
RM_FN int cross_col(int f) { return (0x311102 >> (4 * f)) & 15; }

RM_FN float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }       // a NaN stays NaN, as torch.clamp keeps it

// sh02rgb of one stored value
RM_FN float old01(float x) { return clamp01(C0 * x + 0.5f); }

// ---- the cross: resize_bilinear_u8's taps of one axis; scale = n_in / n_out as the host divides it ----
struct Tap {
    int32_t i0, i1;
    double w;
};

RM_FN Tap cross_tap(int32_t o, int32_t n_in, double scale) {
    const double s = ((double)o + 0.5) * scale - 0.5;
    const double fl = floor(s);
    int32_t i0 = (int32_t)fl;
    int32_t i1 = i0 + 1;
    Tap t;
    t.w = i0 < 0 ? 0.0 : s - fl;
    t.i1 = i1 < 0 ? 0 : (i1 > n_in - 1 ? n_in - 1 : i1);
    t.i0 = i0 < 0 ? 0 : (i0 > n_in - 1 ? n_in - 1 : i0);
    return t;
}

// the four bytes under the taps -> the resized byte
RM_FN uint8_t cross_blend(uint8_t a00, uint8_t a01, uint8_t a10, uint8_t a11, double wx, double wy) {
    const double top = (double)a00 * (1.0 - wx) + (double)a01 * wx;
    const double bot = (double)a10 * (1.0 - wx) + (double)a11 * wx;
    const double v = floor((top * (1.0 - wy) + bot * wy) + 0.5);
    return (uint8_t)(v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v));
}

RM_FN float unit_of_byte(uint8_t b) { return (float)b / 255.0f; }

// ---- the lat-long picture: latlong_to_cubemap's address of the texel (face s, row i, column j), fp64 ----
struct Wrap {
    int32_t i0, i1;
    float w;
};

RM_FN Wrap wrap_tap(double t, int32_t n) {
    const double p = t * (double)n - 0.5;
    const double fl = floor(p);
    int32_t i0 = (int32_t)fl;           // t in [0, 1], so fl in [-1, n]
    if (i0 < 0) i0 += n;
    if (i0 >= n) i0 -= n;
    Wrap r;
    r.i0 = i0;
    r.i1 = i0 + 1 == n ? 0 : i0 + 1;
    r.w = (float)(p - fl);
    return r;
}

RM_FN void latlong_address(int s, int32_t i, int32_t j, int32_t R, int32_t h, int32_t w, Wrap* tx, Wrap* ty) {
    const double gx = (double)(2 * j + 1) / (double)R - 1.0;
    const double gy = (double)(2 * i + 1) / (double)R - 1.0;
    double d0, d1, d2;
    switch (s) {            // cube_to_dir
    case 0: d0 = 1.0; d1 = -gy; d2 = -gx; break;
    case 1: d0 = -1.0; d1 = -gy; d2 = gx; break;
    case 2: d0 = gx; d1 = 1.0; d2 = gy; break;
    case 3: d0 = gx; d1 = -1.0; d2 = -gy; break;
    case 4: d0 = gx; d1 = -gy; d2 = 1.0; break;
    default: d0 = -gx; d1 = -gy; d2 = -1.0; break;
    }
    const double len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const double v0 = d0 / len, v1 = d1 / len, v2 = d2 / len;
    const double c = v1 < -1.0 ? -1.0 : (v1 > 1.0 ? 1.0 : v1);
    const double tu = atan2(v0, -v2) / (2.0 * 3.141592653589793) + 0.5;
    const double tv = acos(c) / 3.141592653589793;
    *tx = wrap_tap(tu, w);
    *ty = wrap_tap(tv, h);
}

RM_FN float latlong_blend(float a00, float a01, float a10, float a11, float wx, float wy) {
    const float top = a00 * (1.0f - wx) + a01 * wx;
    const float bot = a10 * (1.0f - wx) + a11 * wx;
    return top * (1.0f - wy) + bot * wy;
}

// ---- the mode tail, shared by both kernels: x the stored old texel (not read with mode -1), n the picture's value ----
RM_FN void mode_tail(const float x[3], const float n[3], int mode, float out[3]) {
    float v[3] = {n[0], n[1], n[2]};
    if (mode != -1) {
        const float o[3] = {old01(x[0]), old01(x[1]), old01(x[2])};
        if (mode == 0) {
            const float m = ((clamp01(3.0f * o[0]) + clamp01(3.0f * o[1])) + clamp01(3.0f * o[2])) / 3.0f;
            for (int c = 0; c < 3; ++c) v[c] = n[c] * m;
        } else if (mode == 1) {
            for (int c = 0; c < 3; ++c) v[c] = n[c] * o[c];
        } else if (mode == 2) {
            for (int c = 0; c < 3; ++c) v[c] = o[c] / n[c];
        } else {
            const bool lit = ((n[0] + n[1]) + n[2]) > 0.01f;
            const float m2 = 2.0f * (((o[0] + o[1]) + o[2]) / 3.0f);
            for (int c = 0; c < 3; ++c) v[c] = n[c] + (lit ? m2 * n[c] : o[c]);
        }
    }
    for (int c = 0; c < 3; ++c) out[c] = (v[c] - 0.5f) / C0;
}

}  // namespace retexture_math
