// Seamless cubemap sampling (texgs.h "seamless cubemap sampling"): what Texture-GS uses nvdiffrast's dr.texture(..., boundary_mode=
// 'cube') for -- the lat-long picture of the texture (sphere_map) and the chessboard colouring of stage 2.
//
// One query per lane, a loop over the channels, no LDS: a query reads 4 taps x C floats and writes C floats, nothing is shared
// between lanes except through the caches.  The rasterizer's own fetch (render.hip cube_address) clamps to the edge inside a
// face; the face selection and (col, row) below restate its dozen lines, the taps differ.
//
// Seams.  A bilinear tap one texel outside its face ((x, y) with x or y at -1 or R) belongs to the face across that edge.  It is
// found in INTEGERS from a 6 faces x 4 edges table, not by re-projecting the tap's centre: the re-projected centre lies within
// 0.5/(R + 1) texel of a rounding boundary (1.2e-4 at R = 4096), which is the size of the fp32 error of `col` there.  An entry
// holds the neighbour face, the neighbour's edge the two faces share, and whether the index along the edge runs the other way.
// With (s, t) the in-face coordinates in [-1, 1] (col along s, row along t), cube_to_dir (NVDIFFREC/util.py:94-101) is
//     +x: (1, -t, -s)   -x: (-1, -t, s)   +y: (s, 1, t)   -y: (s, -1, -t)   +z: (s, -t, 1)   -z: (-s, -t, -1)
// and e.g. leaving +x over s > 1 makes -z dominant, where s' = -x/|z| -> -1 (its column 0, edge 0) and t' = -y = t (same row, not
// reversed): entry (+x, edge 1) = (-z, edge 0, same).  The other 23 follow the same way.
#include "common.h"
#include "abi_support.h"

#define CT_BLOCK 256

// edges: 0: x = -1, 1: x = R, 2: y = -1, 3: y = R.  Entry = neighbour face | neighbour edge << 3 | reversed << 5, four entries of
// 6 bits per face.
#define CT_E(face, edge, rev) ((uint32_t)((face) | ((edge) << 3) | ((rev) << 5)))
#define CT_FACE(e0, e1, e2, e3) ((e0) | ((e1) << 6) | ((e2) << 12) | ((e3) << 18))
__device__ __forceinline__ uint32_t cube_seam_row(int face) {
    constexpr uint32_t PX = CT_FACE(CT_E(4, 1, 0), CT_E(5, 0, 0), CT_E(2, 1, 1), CT_E(3, 1, 0));
    constexpr uint32_t NX = CT_FACE(CT_E(5, 1, 0), CT_E(4, 0, 0), CT_E(2, 0, 0), CT_E(3, 0, 1));
    constexpr uint32_t PY = CT_FACE(CT_E(1, 2, 0), CT_E(0, 2, 1), CT_E(5, 2, 1), CT_E(4, 2, 0));
    constexpr uint32_t NY = CT_FACE(CT_E(1, 3, 1), CT_E(0, 3, 0), CT_E(4, 3, 0), CT_E(5, 3, 1));
    constexpr uint32_t PZ = CT_FACE(CT_E(1, 1, 0), CT_E(0, 0, 0), CT_E(2, 3, 0), CT_E(3, 2, 0));
    constexpr uint32_t NZ = CT_FACE(CT_E(0, 1, 0), CT_E(1, 0, 0), CT_E(2, 2, 1), CT_E(3, 3, 1));
    return face == 0 ? PX : face == 1 ? NX : face == 2 ? PY : face == 3 ? NY : face == 4 ? PZ : NZ;      // selects, no memory
}

// Texel index ((face R + y) R + x) of tap (x, y), x and y in [-1, R]; -1 for the corner tap that does not exist.
__device__ __forceinline__ int cube_tap_texel(int face, int x, int y, int R) {
    const bool ox = (x < 0) | (x >= R), oy = (y < 0) | (y >= R);
    if (ox & oy) return -1;
    if (ox | oy) {
        const int e = ox ? (x < 0 ? 0 : 1) : (y < 0 ? 2 : 3);
        const int along = ox ? y : x;
        const uint32_t ent = (cube_seam_row(face) >> (6 * e)) & 63u;
        const int ne = (int)((ent >> 3) & 3u);
        const int b = (ent >> 5) ? R - 1 - along : along;
        face = (int)(ent & 7u);
        x = ne == 0 ? 0 : ne == 1 ? R - 1 : b;
        y = ne == 2 ? 0 : ne == 3 ? R - 1 : b;
    }
    return (face * R + y) * R + x;
}

struct CubeQuery {
    bool  ok;                   // false: zero or non-finite direction
    int   axis, face;
    float col, row;
    float sc, tc, ma, sm, su, sv;       // for the backward: col = (sc/ma + 1) R/2 - 0.5 with sc = su * ua, ma = sm * m
};

__device__ __forceinline__ CubeQuery cube_query(float u0, float u1, float u2, int R) {
    CubeQuery q;
    const float a0 = fabsf(u0), a1 = fabsf(u1), a2 = fabsf(u2);
    float m, ua, ub;
    if (a0 >= a1 && a0 >= a2) { q.axis = 0; m = u0; q.sm = (u0 >= 0.f) ? 1.f : -1.f; ua = u2; q.su = -q.sm; ub = u1; q.sv = -1.f; }
    else if (a1 >= a2)        { q.axis = 1; m = u1; q.sm = (u1 >= 0.f) ? 1.f : -1.f; ua = u0; q.su = 1.f;   ub = u2; q.sv = q.sm; }
    else                      { q.axis = 2; m = u2; q.sm = (u2 >= 0.f) ? 1.f : -1.f; ua = u0; q.su = q.sm;  ub = u1; q.sv = -1.f; }
    q.face = 2 * q.axis + (q.sm > 0.f ? 0 : 1);
    q.ma = fabsf(m);
    // finite and non-zero (a NaN fails every comparison, so it also lands here through the last branch above)
    q.ok = (a0 < INFINITY) & (a1 < INFINITY) & (a2 < INFINITY) & (q.ma > 0.f);
    q.sc = q.su * ua; q.tc = q.sv * ub;
    const float halfR = 0.5f * (float)R;
    // a true division: |sc| <= ma, so the quotient is in [-1, 1] for every finite non-zero direction, denormal ones included
    q.col = (q.sc / q.ma + 1.0f) * halfR - 0.5f;
    q.row = (q.tc / q.ma + 1.0f) * halfR - 0.5f;
    return q;
}

struct CubeTaps {
    int   texel[4];             // 00, 10 (x + 1), 01 (y + 1), 11; -1: dropped
    float w[4];                 // final weights (0 for a dropped tap), summing to 1
    float fx, fy, rs;           // rs = 1 / (sum of the kept bilinear weights)
};

__device__ __forceinline__ CubeTaps cube_taps(const CubeQuery& q, int R) {
    CubeTaps t;
    // col is in [-0.5, R - 0.5] up to rounding: the clamp keeps every tap coordinate in [-1, R] whatever the rounding did
    const int x0 = min(max((int)floorf(q.col), -1), R - 1), y0 = min(max((int)floorf(q.row), -1), R - 1);
    t.fx = q.col - (float)x0; t.fy = q.row - (float)y0;
    t.w[0] = (1.f - t.fx) * (1.f - t.fy); t.w[1] = t.fx * (1.f - t.fy); t.w[2] = (1.f - t.fx) * t.fy; t.w[3] = t.fx * t.fy;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.texel[k] = cube_tap_texel(q.face, x0 + (k & 1), y0 + (k >> 1), R);
        if (t.texel[k] < 0) t.w[k] = 0.f;
        s += t.w[k];
    }
    // at most one tap is dropped and its weight is at most 1/4 (the query lies inside the face), so s >= 3/4
    t.rs = 1.0f;
    if (t.texel[0] < 0 || t.texel[1] < 0 || t.texel[2] < 0 || t.texel[3] < 0) {
        t.rs = 1.0f / s;
#pragma unroll
        for (int k = 0; k < 4; ++k) t.w[k] *= t.rs;
    }
    return t;
}

__device__ __forceinline__ int cube_nearest_texel(const CubeQuery& q, int R) {
    const int x = min(max((int)floorf(q.col + 0.5f), 0), R - 1), y = min(max((int)floorf(q.row + 0.5f), 0), R - 1);
    return (q.face * R + y) * R + x;
}

template <bool MAP> __device__ __forceinline__ float cube_tap_value(float t) {
    return MAP ? fminf(fmaxf(fmaf(TG_SH_C0, t, 0.5f), 0.f), 1.f) : t;
}

// One output row: `out` points at its C floats.
template <bool MAP> __device__ __forceinline__ void cube_fetch(const float* __restrict__ tex, int R, int C, float u0, float u1,
                                                                float u2, int filter, float* __restrict__ out) {
    const CubeQuery q = cube_query(u0, u1, u2, R);
    if (!q.ok) {
        for (int c = 0; c < C; ++c) out[c] = 0.f;
        return;
    }
    if (filter == TEXGS_CUBE_NEAREST) {
        const float* p = tex + (size_t)cube_nearest_texel(q, R) * C;
        for (int c = 0; c < C; ++c) out[c] = cube_tap_value<MAP>(p[c]);
        return;
    }
    const CubeTaps t = cube_taps(q, R);
    const float* p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = tex + (size_t)max(t.texel[k], 0) * C;     // a dropped tap reads texel 0 with weight 0
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = cube_tap_value<MAP>(p[k][c]);
            acc += (t.texel[k] >= 0) ? t.w[k] * v : 0.f;          // (0 * inf of a non-finite texel 0 must not leak in)
        }
        out[c] = acc;
    }
}

template <bool MAP> __global__ __launch_bounds__(CT_BLOCK) void k_cube_sample(const float* __restrict__ tex, int R, int C,
                                                                               const float* __restrict__ dirs, int N, int filter,
                                                                               float* __restrict__ out) {
    const int n = (int)(blockIdx.x * CT_BLOCK + threadIdx.x);
    if (n >= N) return;
    const float* d = dirs + (size_t)n * 3;
    cube_fetch<MAP>(tex, R, C, d[0], d[1], d[2], filter, out + (size_t)n * C);
}

// Consecutive lanes take consecutive columns (gx), so a wave's taps fall on neighbouring texels.  The direction is computed in
// double and rounded once: the fetch's error bound leaves the direction a fraction of an fp32 ulp.  The two sinpi/cospi pairs per
// pixel were not timed on their own; the whole kernel takes about 50 us at 512 x 1024 from a 1024^2 texture (profiles/cubetex_bench.json).
template <bool MAP> __global__ __launch_bounds__(CT_BLOCK) void k_cube_latlong(const float* __restrict__ tex, int R, int C, int H,
                                                                                int W, float* __restrict__ out) {
    const int idx = (int)(blockIdx.x * CT_BLOCK + threadIdx.x);
    if (idx >= H * W) return;
    const int i = idx / W, j = idx - i * W;
    // linspace(1/H, 1 - 1/H, H)[i] = (H - 1 + i (H - 2)) / (H (H - 1));  linspace(-1 + 1/W, 1 - 1/W, W)[j] = (2 j + 1 - W) / W
    const double gy = H > 1 ? ((double)(H - 1) + (double)i * (double)(H - 2)) / ((double)H * (double)(H - 1)) : 1.0;
    const double gx = (double)(2 * (long long)j + 1 - W) / (double)W;
    const double st = sinpi(gy), ct = cospi(gy), sp = sinpi(gx), cp = cospi(gx);
    cube_fetch<MAP>(tex, R, C, (float)(st * sp), (float)ct, (float)(-st * cp), TEXGS_CUBE_LINEAR, out + (size_t)idx * C);
}

__global__ __launch_bounds__(CT_BLOCK) void k_cube_sample_bwd(const float* __restrict__ tex, int R, int C,
                                                               const float* __restrict__ dirs, int N, const float* __restrict__ g_out,
                                                               float* __restrict__ d_tex, float* __restrict__ d_dirs) {
    const int n = (int)(blockIdx.x * CT_BLOCK + threadIdx.x);
    if (n >= N) return;
    const float* d = dirs + (size_t)n * 3;
    const CubeQuery q = cube_query(d[0], d[1], d[2], R);
    if (!q.ok) {
        if (d_dirs) { d_dirs[(size_t)n * 3] = 0.f; d_dirs[(size_t)n * 3 + 1] = 0.f; d_dirs[(size_t)n * 3 + 2] = 0.f; }
        return;
    }
    const CubeTaps t = cube_taps(q, R);
    const float* g = g_out + (size_t)n * C;
    float gcol = 0.f, grow = 0.f;
    for (int c = 0; c < C; ++c) {
        const float gc = g[c];
        if (d_tex) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t.texel[k] >= 0) atomicAdd(d_tex + (size_t)t.texel[k] * C + c, t.w[k] * gc);
        }
        if (d_dirs) {
            float v[4], o = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = (t.texel[k] >= 0) ? tex[(size_t)t.texel[k] * C + c] : 0.f;
                o += t.w[k] * v[k];
            }
            // out = sum_k w_k T_k / S with S = 1 - w_dropped: d out = (sum_{k kept} dw_k T_k + out dw_dropped) / S, which is the plain
            // bilinear derivative with the output standing in for the missing texel
#pragma unroll
            for (int k = 0; k < 4; ++k) if (t.texel[k] < 0) v[k] = o;
            gcol += gc * ((1.f - t.fy) * (v[1] - v[0]) + t.fy * (v[3] - v[2]));
            grow += gc * ((1.f - t.fx) * (v[2] - v[0]) + t.fx * (v[3] - v[1]));
        }
    }
    if (d_dirs) {
        gcol *= t.rs; grow *= t.rs;
        const float h = 0.5f * (float)R / q.ma;                  // d col / d sc
        const float da = gcol * q.su * h, db = grow * q.sv * h;
        const float dm = -(gcol * q.sc + grow * q.tc) * (h / q.ma) * q.sm;
        float r0, r1, r2;
        if (q.axis == 0)      { r0 = dm; r2 = da; r1 = db; }
        else if (q.axis == 1) { r1 = dm; r0 = da; r2 = db; }
        else                  { r2 = dm; r0 = da; r1 = db; }
        float* o = d_dirs + (size_t)n * 3;
        o[0] = r0; o[1] = r1; o[2] = r2;
    }
}

__global__ __launch_bounds__(CT_BLOCK) void k_cube_nearest_bwd(int R, int C, const float* __restrict__ dirs, int N,
                                                                const float* __restrict__ g_out, float* __restrict__ d_tex) {
    const int n = (int)(blockIdx.x * CT_BLOCK + threadIdx.x);
    if (n >= N) return;
    const float* d = dirs + (size_t)n * 3;
    const CubeQuery q = cube_query(d[0], d[1], d[2], R);
    if (!q.ok) return;
    float* p = d_tex + (size_t)cube_nearest_texel(q, R) * C;
    const float* g = g_out + (size_t)n * C;
    for (int c = 0; c < C; ++c) atomicAdd(p + c, g[c]);
}

static inline uint32_t ct_blocks(long long n) { return (uint32_t)((n + CT_BLOCK - 1) / CT_BLOCK); }

static hipError_t launch_cube_sample(const float* tex, int R, int C, const float* dirs, int N, int filter, int tap_map, float* out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    if (tap_map) hipLaunchKernelGGL(k_cube_sample<true>, dim3(ct_blocks(N)), dim3(CT_BLOCK), 0, s, tex, R, C, dirs, N, filter, out);
    else         hipLaunchKernelGGL(k_cube_sample<false>, dim3(ct_blocks(N)), dim3(CT_BLOCK), 0, s, tex, R, C, dirs, N, filter, out);
    return hipGetLastError();
}

static hipError_t launch_cube_latlong(const float* tex, int R, int C, int H, int W, int tap_map, float* out, hipStream_t s) {
    const uint32_t nb = ct_blocks((long long)H * W);
    if (tap_map) hipLaunchKernelGGL(k_cube_latlong<true>, dim3(nb), dim3(CT_BLOCK), 0, s, tex, R, C, H, W, out);
    else         hipLaunchKernelGGL(k_cube_latlong<false>, dim3(nb), dim3(CT_BLOCK), 0, s, tex, R, C, H, W, out);
    return hipGetLastError();
}

static hipError_t launch_cube_sample_backward(const float* tex, int R, int C, const float* dirs, int N, const float* g_out, float* d_tex,
                                float* d_dirs, hipStream_t s) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cube_sample_bwd, dim3(ct_blocks(N)), dim3(CT_BLOCK), 0, s, tex, R, C, dirs, N, g_out, d_tex, d_dirs);
    return hipGetLastError();
}

static hipError_t launch_cube_sample_nearest_backward(int R, int C, const float* dirs, int N, const float* g_out, float* d_tex, hipStream_t s) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cube_nearest_bwd, dim3(ct_blocks(N)), dim3(CT_BLOCK), 0, s, R, C, dirs, N, g_out, d_tex);
    return hipGetLastError();
}

extern "C" {

static int cube_shape_ok(int32_t R, int32_t C) {
    if (R < 2) return fail_msg("R < 2: a cubemap face needs at least 2 x 2 texels");
    if (C < 1) return fail_msg("C < 1");
    if (6ll * R * R * C >= (1ll << 31)) return fail_msg("6 R R C must be below 2^31");
    return 0;
}

int texgs_cube_sample(const float* tex, int32_t R, int32_t C, const float* dirs, int32_t N, int32_t filter, int32_t tap_map,
                      float* out, void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (filter != TEXGS_CUBE_LINEAR && filter != TEXGS_CUBE_NEAREST) return fail_msg("filter must be TEXGS_CUBE_LINEAR or TEXGS_CUBE_NEAREST");
    if (!tex || (N > 0 && (!dirs || !out))) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_sample", launch_cube_sample(tex, R, C, dirs, N, filter, tap_map, out, s), s, false);
}

int texgs_cube_latlong(const float* tex, int32_t R, int32_t C, int32_t H, int32_t W, int32_t tap_map, float* out, void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (H < 1 || W < 1) return fail_msg("H and W must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("H W must be below 2^31");
    if (!tex || !out) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_latlong", launch_cube_latlong(tex, R, C, H, W, tap_map, out, s), s, false);
}

int texgs_cube_sample_backward(const float* tex, int32_t R, int32_t C, const float* dirs, int32_t N, const float* g_out,
                               float* d_tex, float* d_dirs, void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (!d_tex && !d_dirs) return fail_msg("d_tex and d_dirs are both NULL: nothing to compute");
    if ((d_dirs && !tex) || (N > 0 && (!dirs || !g_out))) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_sample_backward", launch_cube_sample_backward(tex, R, C, dirs, N, g_out, d_tex, d_dirs, s), s, false);
}

int texgs_cube_sample_nearest_backward(int32_t R, int32_t C, const float* dirs, int32_t N, const float* g_out, float* d_tex,
                                       void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (!d_tex || (N > 0 && (!dirs || !g_out))) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_sample_nearest_backward", launch_cube_sample_nearest_backward(R, C, dirs, N, g_out, d_tex, s), s, false);
}

}  // extern "C"
