// The texture-gradient RECORD codec and the fixed-point scale of the bin reduce (render.hip: K7 packs, k_texgrad_reduce unpacks and
// sums; tests/texrec_ref.py states both again in numpy), kept apart from the kernels so that the same text compiles for the host:
// tests/test_texrec_host.py builds it with g++ and compares it bit for bit with the numpy statement, on a machine without a GPU.
// render.hip is built with -ffp-contract=fast and the host harness with -ffp-contract=off; nothing here depends on which:
//   * fx * 262144 + 0.5 (rec_word0): the product is a scaling by a power of two, exact, so the fused and the unfused form round the
//     same real number once;
//   * w * dx (contribution): w has at most 24 significant bits and dx = x * 2^k is exact in double with at most 24, a 48-bit product,
//     exact in double -- adding the magic number rounds the same real number once, fused or not;
//   * the tap weights are products of two floats converted to double at once: there is no addition to fuse them with.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TR_FN __host__ __device__ __forceinline__
#else
#define TR_FN inline
#endif

namespace texrec_math {

constexpr float C0 = 0.28209479177387814f;      // TG_SH_C0: |record value| <= C0 * max |dL/dpixel colour|

TR_FN uint32_t bits_of(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
TR_FN float float_of(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
TR_FN long long bits_of(double v) { long long u; __builtin_memcpy(&u, &v, 8); return u; }

// Record, 16 bytes, one per bilinear footprint:
//   a = low 16 bits of fx18 | low 16 bits of fy18 << 16          fx18 = round(fx * 2^18), clamped to 2^18 - 1
//   b = r, its 5 low mantissa bits replaced by the footprint's cell x inside its 32x32-texel bin (r rounded to 18 mantissa bits)
//   c = g, likewise with cell y          d = b, its 4 low mantissa bits = the two high bits of fx18 and of fy18
struct alignas(16) Rec4 { uint32_t a, b, c, d; };
struct RecVal { int cx, cy; float fx, fy, x0, x1, x2; };

TR_FN uint32_t rec_word0(float fx, float fy, uint32_t& hi) {
    const uint32_t rx = (uint32_t)(fx * 262144.0f + 0.5f), ry = (uint32_t)(fy * 262144.0f + 0.5f);
    const uint32_t qx = rx < 262143u ? rx : 262143u, qy = ry < 262143u ? ry : 262143u;
    hi = (qx >> 16) | ((qy >> 16) << 2);
    return (qx & 0xFFFFu) | (qy << 16);
}

// A colour value with its `mask` low mantissa bits (31 or 15) cleared for the payload: a finite value is rounded to the nearest kept
// value, ties away from zero (the add carries into the exponent where it must: the largest finite values round to inf).  inf / NaN
// take no rounding add -- it would carry out of the exponent field (0x7FFFFFFF -> -0.0) -- inf stays inf, and a NaN whose payload sits
// in the dropped bits alone keeps it five bits higher, so that every NaN stays a NaN.
TR_FN uint32_t rec_round(uint32_t bits, uint32_t mask) {
    const bool nonfinite = (bits & 0x7F800000u) == 0x7F800000u;
    const uint32_t v = nonfinite ? (bits | ((bits & mask) << 5)) : bits + ((mask + 1u) >> 1);
    return v & ~mask;
}

TR_FN Rec4 rec_pack(uint32_t w0, uint32_t hi, int cx, int cy, float x0, float x1, float x2) {
    Rec4 r;
    r.a = w0;
    r.b = rec_round(bits_of(x0), 31u) | (uint32_t)(cx & 31);
    r.c = rec_round(bits_of(x1), 31u) | (uint32_t)(cy & 31);
    r.d = rec_round(bits_of(x2), 15u) | hi;
    return r;
}

TR_FN RecVal rec_unpack(const Rec4 w) {
    RecVal r;
    r.fx = (float)((w.a & 0xFFFFu) | ((w.d & 3u) << 16)) * (1.0f / 262144.0f);
    r.fy = (float)((w.a >> 16) | (((w.d >> 2) & 3u) << 16)) * (1.0f / 262144.0f);
    r.cx = (int)(w.b & 31u); r.cy = (int)(w.c & 31u);
    r.x0 = float_of(w.b & ~31u); r.x1 = float_of(w.c & ~31u); r.x2 = float_of(w.d & ~15u);
    return r;
}

// The reduce's scale from the bits of max |dL/dpixel colour| of the call: bound = C0 * that, 2^(e-1) <= bound < 2^e, and a record
// value times `up` = 2^(42-e) is below 2^42 in magnitude.  up and down are DOUBLES (float 2^(42-e) is inf from e = -86 down, float
// 2^(e-42) is 0 from e = -108 down): finite and non-zero for every finite bound, up * down = 1.  A bound of 0 (no gradient, or
// one that C0 rounds to 0) has e = 0; every record of such a call is 0.
struct Scale { bool nonfinite; int e; double up, down; };

TR_FN Scale scale_of(uint32_t bbits) {
    Scale s;
    s.nonfinite = bbits >= 0x7F800000u;
    s.e = 0; s.up = 0.0; s.down = 0.0;
    if (s.nonfinite) return s;
    const float bound = C0 * float_of(bbits);
    (void)frexpf(bound, &s.e);                                 // bound < 2^e
    s.up = ldexp(1.0, 42 - s.e);
    s.down = ldexp(1.0, s.e - 42);
    return s;
}

// The four tap weights of a record, as the reduce forms them: one float rounding each (fx, fy are multiples of 2^-18, so 1 - fx is
// exact)
TR_FN void tap_weights(float fx, float fy, double w[4]) {
    w[0] = (double)((1.f - fx) * (1.f - fy)); w[1] = (double)(fx * (1.f - fy));
    w[2] = (double)((1.f - fx) * fy); w[3] = (double)(fx * fy);
}

// One tap contribution -> 2^(e-42) fixed point.  float -> int64 without the 11-instruction generic conversion: |v| < 2^42, so
// v + 1.5 * 2^52 (exact in double) carries round(v) in its mantissa; subtracting the bias as integers leaves the two's-complement
// value
TR_FN long long to_fixed(double w, double dx) {
    const double magic = 6755399441055744.0;
    return bits_of(w * dx + magic) - bits_of(magic);
}

// A tile texel's sum back to float: the int64 rounds to float once, the scaling is exact in double, and the last conversion is
// exact unless the result is a float denormal (one more rounding there)
TR_FN float from_fixed(long long q, double down) { return (float)((double)(float)q * down); }

}  // namespace texrec_math
