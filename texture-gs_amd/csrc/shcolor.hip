// The colour stage (include/texgs_shcolor.h): SH coefficients of degree 0..4 and the view direction -> colors_precomp, and its
// backward -- what the reference runs as a chain of some sixty elementwise torch launches per view under convert_SHs_python.
// Built with -ffp-contract=off: the row arithmetic (shcolor_math.h) is compared bit for bit with tests/shcolor_ref.py.
//
// One thread per Gaussian, SB = 128 rows per workgroup.  The stage is bound by the coefficient rows (12 K bytes per Gaussian against
// 12 for the means and 12 per view for the colour), so those move as dense dwords: the workgroup reads its rows' active coefficients
// cooperatively into LDS (consecutive lanes, consecutive addresses; a lane per row would touch 64 lines per instruction), each thread
// then walks its own row, whose LDS stride is odd (3 A | 1 floats) so that the 32 lanes of a ds_read_b32 group hit 32 banks.
//   * forward: the rows are staged once, then the views of the launch are walked; every view's colour is three dwords per lane.
//   * backward: the rows are staged once; the gradient row (3 A floats) lives in registers over the views, summed in view order;
//     it then overwrites the thread's own LDS row and the workgroup writes the rows out densely, once, zeros for the inactive
//     coefficients included.  d_xyz is written once.
// 128 rows, not 256: at K = 25 a row is 300 bytes and 256 of them (76.8 KB) are past the 64 KB a workgroup gets; 128 rows are
// 38.4 KB at degree 4 and 25 KB at degree 3.  The degree-4 FORWARD is the exception: 256 rows staged in two passes
// (k_sh_colors_deg4 below), which measured faster; the backward keeps a row's 25 t_k together and stays one pass.  The degree is a
// template argument (every basis index a constant); the layout, the mode and K are wave-uniform run-time values.  Offsets are 64-bit.
#include "common.h"
#include "abi_support.h"
#include "texgs_shcolor.h"
#include "shcolor_math.h"

namespace {

namespace sm = shcolor_math;
constexpr int SB = TEXGS_SH_COLORS_ROWS_PER_WORKGROUP;
constexpr int SV = TEXGS_SH_COLORS_MAX_VIEWS;
static_assert(SB % 64 == 0, "whole waves");

constexpr int row_width(int deg) { return 3 * sm::coeffs_of(deg); }
constexpr int row_stride(int deg) { return row_width(deg) | 1; }           // odd: conflict-free for a lane per row

struct ShColorsArgs {
    TexGSShColors c;
    TexGSShColorView v[SV];
    int32_t count;
};

struct ShColorsGradArgs {
    TexGSShColorsGrad g;
    TexGSShColorGradView v[SV];
    int32_t count;
};

// Coefficients [K0, K0 + KB) of the workgroup's `rows` rows (from row0 on) into LDS as [row][k - K0][c], stride LS, whatever the
// source layout; NT threads.  Nothing outside the band is read.
template <uint32_t K0, uint32_t KB, uint32_t LS, uint32_t NT>
__device__ __forceinline__ void stage_band(const float* __restrict__ sh, const float* __restrict__ dc, const float* __restrict__ rest,
                                           int K, int layout, float* s, size_t row0, uint32_t rows) {
    constexpr uint32_t W = 3 * KB;
    const uint32_t K3 = 3u * (uint32_t)K;
    if (sh) {
        const float* base = sh + row0 * K3;
        if (layout == TEXGS_SH_LAYOUT_KC) {
            for (uint32_t i = threadIdx.x; i < rows * W; i += NT) {
                const uint32_t r = i / W, j = i - r * W;
                s[r * LS + j] = base[(size_t)r * K3 + 3 * K0 + j];
            }
        } else {
            for (uint32_t i = threadIdx.x; i < rows * K3; i += NT) {
                const uint32_t r = i / K3, j = i - r * K3, c = j / (uint32_t)K, k = j - c * (uint32_t)K;
                if (k >= K0 && k < K0 + KB) s[r * LS + 3 * (k - K0) + c] = base[i];
            }
        }
    } else {
        constexpr uint32_t DC = K0 == 0 ? 3 : 0;            // the band's floats that come from sh_dc
        constexpr uint32_t WR = W - DC, C0R = K0 == 0 ? 0 : 3 * (K0 - 1);          // ... and from sh_rest, from its column C0R on
        if constexpr (DC > 0) {
            const float* b0 = dc + row0 * 3;
            for (uint32_t i = threadIdx.x; i < rows * 3; i += NT) {
                const uint32_t r = i / 3, j = i - r * 3;
                s[r * LS + j] = b0[i];
            }
        }
        if constexpr (WR > 0) {
            const uint32_t R3 = K3 - 3;
            const float* b1 = rest + row0 * R3;
            for (uint32_t i = threadIdx.x; i < rows * WR; i += NT) {
                const uint32_t r = i / WR, j = i - r * WR;
                s[r * LS + DC + j] = b1[(size_t)r * R3 + C0R + j];
            }
        }
    }
}

template <int DEG>
__device__ __forceinline__ void stage_rows(const float* __restrict__ sh, const float* __restrict__ dc, const float* __restrict__ rest,
                                           int K, int layout, float* s, size_t row0, uint32_t rows) {
    stage_band<0, sm::coeffs_of(DEG), row_stride(DEG), SB>(sh, dc, rest, K, layout, s, row0, rows);
}

// `width` active floats of every LDS row (from LDS column `col` on) to rows of `stride` floats at dst, then zeros for the rest of
// each row: dense dwords
template <uint32_t WIDTH>
__device__ __forceinline__ void rows_out(float* __restrict__ dst, const float* s, uint32_t ls, uint32_t col, uint32_t stride, uint32_t rows) {
    if constexpr (WIDTH > 0) {
        for (uint32_t i = threadIdx.x; i < rows * WIDTH; i += SB) {
            const uint32_t r = i / WIDTH, j = i - r * WIDTH;
            dst[(size_t)r * stride + j] = s[r * ls + col + j];
        }
    }
    const uint32_t wz = stride - WIDTH;
    if (wz) {
        for (uint32_t i = threadIdx.x; i < rows * wz; i += SB) {
            const uint32_t r = i / wz, j = i - r * wz;
            dst[(size_t)r * stride + WIDTH + j] = 0.0f;
        }
    }
}

template <int DEG>
__global__ void __launch_bounds__(SB)
k_sh_colors(ShColorsArgs a) {
    constexpr int LS = row_stride(DEG);
    __shared__ float s_sh[SB * LS];
    const TexGSShColors& c = a.c;
    const size_t row0 = (size_t)blockIdx.x * SB;
    const uint32_t rows = (size_t)c.n - row0 < (size_t)SB ? (uint32_t)((size_t)c.n - row0) : (uint32_t)SB;
    stage_rows<DEG>(c.sh, c.sh_dc, c.sh_rest, c.coeffs, c.layout, s_sh, row0, rows);
    __syncthreads();
    if (threadIdx.x >= rows) return;
    const size_t i = row0 + threadIdx.x;
    const float* my = s_sh + threadIdx.x * LS;
    const bool eval_mode = c.mode == TEXGS_SH_EVAL;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (DEG >= 1) { p[0] = c.xyz[3 * i]; p[1] = c.xyz[3 * i + 1]; p[2] = c.xyz[3 * i + 2]; }
    for (int v = 0; v < a.count; ++v) {
        float cam[3] = {0.0f, 0.0f, 0.0f}, out[3];
        if (DEG >= 1 && !eval_mode) {
            const float* __restrict__ cp = a.v[v].campos;
            cam[0] = cp[0]; cam[1] = cp[1]; cam[2] = cp[2];
        }
        sm::row_forward<DEG>(my, p, cam, eval_mode, out);
        float* __restrict__ o = a.v[v].colors + 3 * i;
        o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    }
}

// Degree 4, forward: 256 rows per workgroup, the row staged in two passes -- coefficients 0..15 (48 floats, stride 49: 50 KB), then
// 16..24 (27 floats) -- with the views' running sums in registers between them (the view loop is unrolled: every index a constant).
// The same operation order as sm::row_forward, so the same bits.  One pass over 128 rows of 75 floats holds 300 bytes of LDS per
// thread and two waves per SIMD; this holds 196 and three, and measured 0.31 against 0.39 ms at N = 3 000 000.
constexpr int SP = TEXGS_SH_COLORS_ROWS_PER_WORKGROUP_DEG4;
constexpr uint32_t P1 = 16, P2 = 9, PLS = 3 * P1 + 1;

__device__ __forceinline__ void deg4_basis(const float p[3], const float* __restrict__ cp, bool eval_mode, float b[25]) {
    float d[3];
    if (eval_mode) {
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
    } else {
        const float cam[3] = {cp[0], cp[1], cp[2]};
        sm::direction(p, cam, d);
    }
    sm::basis<4>(d[0], d[1], d[2], b);
}

__global__ void __launch_bounds__(SP)
k_sh_colors_deg4(ShColorsArgs a) {
    __shared__ float s_sh[SP * PLS];
    const TexGSShColors& c = a.c;
    const size_t row0 = (size_t)blockIdx.x * SP;
    const uint32_t rows = (size_t)c.n - row0 < (size_t)SP ? (uint32_t)((size_t)c.n - row0) : (uint32_t)SP;
    const bool live = threadIdx.x < rows;
    const bool eval_mode = c.mode == TEXGS_SH_EVAL;
    const size_t i = row0 + threadIdx.x;
    const float* my = s_sh + threadIdx.x * PLS;
    float p[3] = {0.0f, 0.0f, 0.0f}, acc[SV][3];
    if (live) { p[0] = c.xyz[3 * i]; p[1] = c.xyz[3 * i + 1]; p[2] = c.xyz[3 * i + 2]; }
    stage_band<0, P1, PLS, SP>(c.sh, c.sh_dc, c.sh_rest, c.coeffs, c.layout, s_sh, row0, rows);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < SV; ++v) {
        if (live && v < a.count) {
            float b[25];
            deg4_basis(p, a.v[v].campos, eval_mode, b);
            for (int ch = 0; ch < 3; ++ch) acc[v][ch] = b[0] * my[ch];
#pragma unroll
            for (int k = 1; k < (int)P1; ++k)
                for (int ch = 0; ch < 3; ++ch) acc[v][ch] = acc[v][ch] + b[k] * my[3 * k + ch];
        }
    }
    __syncthreads();            // every thread has read its first band
    stage_band<P1, P2, PLS, SP>(c.sh, c.sh_dc, c.sh_rest, c.coeffs, c.layout, s_sh, row0, rows);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < SV; ++v) {
        if (live && v < a.count) {
            float b[25];
            deg4_basis(p, a.v[v].campos, eval_mode, b);
#pragma unroll
            for (int k = (int)P1; k < 25; ++k)
                for (int ch = 0; ch < 3; ++ch) acc[v][ch] = acc[v][ch] + b[k] * my[3 * (k - (int)P1) + ch];
            float* __restrict__ o = a.v[v].colors + 3 * i;
            for (int ch = 0; ch < 3; ++ch) o[ch] = eval_mode ? acc[v][ch] : sm::clamp_colour(acc[v][ch]);
        }
    }
}

// what the outputs hold for row i, coefficient k, channel c (the start of the sums of an accumulating call)
__device__ __forceinline__ float previous(const TexGSShColorsGrad& g, size_t i, int k, int c) {
    const size_t K = (size_t)g.coeffs;
    if (g.d_sh) return g.layout == TEXGS_SH_LAYOUT_KC ? g.d_sh[(i * K + k) * 3 + c] : g.d_sh[(i * 3 + c) * K + k];
    if (k == 0) return g.d_sh_dc ? g.d_sh_dc[i * 3 + c] : 0.0f;
    return g.d_sh_rest ? g.d_sh_rest[(i * (K - 1) + (k - 1)) * 3 + c] : 0.0f;
}

template <int DEG>
__global__ void __launch_bounds__(SB)
k_sh_colors_backward(ShColorsGradArgs a) {
    constexpr int KA = sm::coeffs_of(DEG), W = row_width(DEG), LS = row_stride(DEG);
    __shared__ float s_sh[SB * LS];             // the SH rows, then the gradient rows
    const TexGSShColorsGrad& g = a.g;
    const size_t row0 = (size_t)blockIdx.x * SB;
    const uint32_t rows = (size_t)g.n - row0 < (size_t)SB ? (uint32_t)((size_t)g.n - row0) : (uint32_t)SB;
    stage_rows<DEG>(g.sh, g.sh_dc, g.sh_rest, g.coeffs, g.layout, s_sh, row0, rows);
    __syncthreads();
    const bool want_sh = g.d_sh || g.d_sh_dc || g.d_sh_rest;           // (uniform: kernel arguments)
    const bool want_xyz = g.d_xyz != nullptr;
    const bool eval_mode = g.mode == TEXGS_SH_EVAL;
    float* my = s_sh + threadIdx.x * LS;
    if (threadIdx.x < rows) {
        const size_t i = row0 + threadIdx.x;
        float acc[W], ax[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] = 0.0f;
        if (g.accumulate) {
            if (want_sh) {
#pragma unroll
                for (int k = 0; k < KA; ++k)
                    for (int c = 0; c < 3; ++c) acc[3 * k + c] = previous(g, i, k, c);
            }
            if (want_xyz) { ax[0] = g.d_xyz[3 * i]; ax[1] = g.d_xyz[3 * i + 1]; ax[2] = g.d_xyz[3 * i + 2]; }
        }
        float p[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (DEG >= 1) { p[0] = g.xyz[3 * i]; p[1] = g.xyz[3 * i + 1]; p[2] = g.xyz[3 * i + 2]; }
        for (int v = 0; v < a.count; ++v) {
            float cam[3] = {0.0f, 0.0f, 0.0f};
            if (DEG >= 1 && !eval_mode) {
                const float* __restrict__ cp = a.v[v].campos;
                cam[0] = cp[0]; cam[1] = cp[1]; cam[2] = cp[2];
            }
            const float* __restrict__ gp = a.v[v].g_colors + 3 * i;
            const float up[3] = {gp[0], gp[1], gp[2]};
            sm::row_backward_view<DEG>(my, p, cam, up, eval_mode, want_sh, want_xyz, acc, ax);
        }
        if (want_xyz) { g.d_xyz[3 * i] = ax[0]; g.d_xyz[3 * i + 1] = ax[1]; g.d_xyz[3 * i + 2] = ax[2]; }
        if (want_sh) {          // the thread's own row: read above, by it alone
#pragma unroll
            for (int j = 0; j < W; ++j) my[j] = acc[j];
        }
    }
    if (!want_sh) return;
    __syncthreads();
    const uint32_t K = (uint32_t)g.coeffs, K3 = 3 * K;
    if (g.d_sh) {
        float* base = g.d_sh + row0 * K3;
        if (g.layout == TEXGS_SH_LAYOUT_KC) {
            rows_out<W>(base, s_sh, LS, 0, K3, rows);
        } else {
            for (uint32_t i = threadIdx.x; i < rows * K3; i += SB) {
                const uint32_t r = i / K3, j = i - r * K3, c = j / K, k = j - c * K;
                base[i] = k < (uint32_t)KA ? s_sh[r * LS + 3 * k + c] : 0.0f;
            }
        }
    } else {
        if (g.d_sh_dc) rows_out<3>(g.d_sh_dc + row0 * 3, s_sh, LS, 0, 3, rows);
        if (g.d_sh_rest && K > 1) rows_out<W - 3>(g.d_sh_rest + row0 * (K3 - 3), s_sh, LS, 3, K3 - 3, rows);
    }
}

inline uint32_t sh_groups(int32_t n) { return ((uint32_t)n + SB - 1) / SB; }

}  // namespace

// 1 <= count <= TEXGS_SH_COLORS_MAX_VIEWS, n >= 1 and everything else validated by check_sh_colors and the entry points below
static hipError_t launch_sh_colors(const TexGSShColors* c, const TexGSShColorView* views, int count, hipStream_t s) {
    ShColorsArgs a;
    a.c = *c;
    for (int k = 0; k < SV; ++k) a.v[k] = k < count ? views[k] : TexGSShColorView{nullptr, nullptr};
    a.count = count;
    const dim3 grid(sh_groups(c->n)), block(SB);
    switch (c->degree) {
        case 0: hipLaunchKernelGGL(k_sh_colors<0>, grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL(k_sh_colors<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_sh_colors<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_sh_colors<3>, grid, block, 0, s, a); break;
#ifdef TEXGS_SH_COLORS_BUILD_ONE_PASS        // the alternative that was measured and is not built: 128 rows, the whole row in one pass
        case 4: hipLaunchKernelGGL(k_sh_colors<4>, grid, block, 0, s, a); break;
#else
        case 4: hipLaunchKernelGGL(k_sh_colors_deg4, dim3(((uint32_t)c->n + SP - 1) / SP), dim3(SP), 0, s, a); break;
#endif
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

static hipError_t launch_sh_colors_backward(const TexGSShColorsGrad* g, const TexGSShColorGradView* views, int count, hipStream_t s) {
    ShColorsGradArgs a;
    a.g = *g;
    for (int k = 0; k < SV; ++k) a.v[k] = k < count ? views[k] : TexGSShColorGradView{nullptr, nullptr};
    a.count = count;
    const dim3 grid(sh_groups(g->n)), block(SB);
    switch (g->degree) {
        case 0: hipLaunchKernelGGL(k_sh_colors_backward<0>, grid, block, 0, s, a); break;
        case 1: hipLaunchKernelGGL(k_sh_colors_backward<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(k_sh_colors_backward<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(k_sh_colors_backward<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(k_sh_colors_backward<4>, grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" {

// include/texgs_shcolor.h: every argument is checked before the launch, so a refused call has changed nothing
static int check_sh_colors(int32_t n, int32_t coeffs, int32_t degree, int32_t layout, int32_t mode, int32_t count, const void* sh,
                           const void* sh_dc, const void* sh_rest, const void* views) {
    if (degree < 0 || degree > TEXGS_SH_COLORS_MAX_DEGREE) return fail_msg("degree must be in [0,4]");
    if (coeffs != 1 && coeffs != 4 && coeffs != 9 && coeffs != 16 && coeffs != 25) return fail_msg("coeffs must be 1, 4, 9, 16 or 25");
    if ((degree + 1) * (degree + 1) > coeffs) return fail_msg("(degree + 1)^2 exceeds coeffs");
    if (n < 0) return fail_msg("n < 0");
    if ((int64_t)n * coeffs * 3 >= (1ll << 31)) return fail_msg("n * coeffs * 3 must be below 2^31");
    if (layout != TEXGS_SH_LAYOUT_KC && layout != TEXGS_SH_LAYOUT_CK) return fail_msg("layout must be 0 ([n,coeffs,3]) or 1 ([n,3,coeffs])");
    if (mode != TEXGS_SH_COLORS && mode != TEXGS_SH_EVAL) return fail_msg("mode must be 0 (colours) or 1 (eval_sh)");
    if (count < 1) return fail_msg("count < 1: at least one view");
    if (count > TEXGS_SH_COLORS_MAX_VIEWS) return fail_msg("count exceeds TEXGS_SH_COLORS_MAX_VIEWS: several calls");
    if (mode == TEXGS_SH_EVAL && count != 1) return fail_msg("mode eval_sh takes exactly one view");
    if (!views) return fail_msg("NULL argument (views)");
    if (sh && (sh_dc || sh_rest)) return fail_msg("both sh and the pair (sh_dc, sh_rest) are set");
    if (!sh && layout != TEXGS_SH_LAYOUT_KC) return fail_msg("the pair (sh_dc, sh_rest) has layout 0 only");
    if (n == 0) return 0;
    if (!sh && !sh_dc) return fail_msg("NULL argument (sh, or sh_dc of the pair)");
    if (!sh && !sh_rest && degree > 0) return fail_msg("NULL argument (sh_rest: read at degree >= 1)");
    if (((uintptr_t)sh | (uintptr_t)sh_dc | (uintptr_t)sh_rest) & 3) return fail_msg("sh, sh_dc and sh_rest must be 4-byte aligned");
    return 0;
}

int texgs_sh_colors_forward(const TexGSShColors* c, const TexGSShColorView* views, int32_t count, void* stream) {
    if (!c) return fail_msg("sh colours descriptor is NULL");
    if (int r = check_sh_colors(c->n, c->coeffs, c->degree, c->layout, c->mode, count, c->sh, c->sh_dc, c->sh_rest, views)) return r;
    if (c->n == 0) return 0;
    if (c->degree > 0 && !c->xyz) return fail_msg("NULL argument (xyz: read at degree >= 1)");
    if ((uintptr_t)c->xyz & 3) return fail_msg("xyz must be 4-byte aligned");
    for (int v = 0; v < count; ++v) {
        if (!views[v].colors) return fail_msg("NULL argument (a view's colors)");
        if (c->degree > 0 && c->mode == TEXGS_SH_COLORS && !views[v].campos) return fail_msg("NULL argument (a view's campos: read at degree >= 1)");
        if (((uintptr_t)views[v].colors | (uintptr_t)views[v].campos) & 3) return fail_msg("a view's campos and colors must be 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    return launched("sh_colors_forward", launch_sh_colors(c, views, count, s), s, false);
}

int texgs_sh_colors_backward(const TexGSShColorsGrad* g, const TexGSShColorGradView* views, int32_t count, void* stream) {
    if (!g) return fail_msg("sh colours backward descriptor is NULL");
    if (int r = check_sh_colors(g->n, g->coeffs, g->degree, g->layout, g->mode, count, g->sh, g->sh_dc, g->sh_rest, views)) return r;
    if (g->accumulate != 0 && g->accumulate != 1) return fail_msg("accumulate must be 0 or 1");
    if (g->n == 0) return 0;
    if (!g->d_sh && !g->d_sh_dc && !g->d_sh_rest && !g->d_xyz)
        return fail_msg("no output requested (d_sh, d_sh_dc, d_sh_rest and d_xyz are all NULL)");
    if (g->d_sh && !g->sh) return fail_msg("d_sh belongs to sh, which is NULL");
    if ((g->d_sh_dc || g->d_sh_rest) && g->sh) return fail_msg("d_sh_dc and d_sh_rest belong to the pair, but sh is set");
    if (g->degree > 0 && !g->xyz) return fail_msg("NULL argument (xyz: read at degree >= 1)");
    if (((uintptr_t)g->xyz | (uintptr_t)g->d_sh | (uintptr_t)g->d_sh_dc | (uintptr_t)g->d_sh_rest | (uintptr_t)g->d_xyz) & 3)
        return fail_msg("xyz, d_sh, d_sh_dc, d_sh_rest and d_xyz must be 4-byte aligned");
    for (int v = 0; v < count; ++v) {
        if (!views[v].g_colors) return fail_msg("NULL argument (a view's g_colors)");
        if (g->degree > 0 && g->mode == TEXGS_SH_COLORS && !views[v].campos) return fail_msg("NULL argument (a view's campos: read at degree >= 1)");
        if (((uintptr_t)views[v].g_colors | (uintptr_t)views[v].campos) & 3) return fail_msg("a view's campos and g_colors must be 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    return launched("sh_colors_backward", launch_sh_colors_backward(g, views, count, s), s, false);
}

}  // extern "C"
