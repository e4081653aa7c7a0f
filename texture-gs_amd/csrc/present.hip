// The output stage (include/texgs_present.h): the rasterizer's maps as something a person looks at, each as one streaming pass.
//   k_present       clamp / 0.5 (n + 1) / composite over a background -> 8-bit [H,W,3|4], f32 [H,W,4], f32 [3,H,W]
//                   (retexture.py:28-32, viewer_renderer.py:138-173, the clamp lines of train.py:58-71)
//   k_depth_range   per-workgroup (min, max) of the depth under the mask          } train.py:22-37,
//   k_depth_colour  re-reduces those partials, normalises, looks the LUT up       } viewer_renderer.py:150-165
//   k_cube_cross    SH-DC cubemap [6,R,R,3] -> 8-bit cross [3R,4R,3], empty cells included (texture_gaussian3d.py:451-461 and
//                   extract_texture.py:17)
// The arithmetic is a bit-exact contract (tests/present_ref.py): the unit is built with -ffp-contract=off, every operation below is
// rounded once, the divisions are IEEE.
//
// Layout.  Everything is indexed by the flat pixel number; planar [C,H,W] and interleaved [H,W,c] are both contiguous in it, so there
// are no row edges.  A thread takes a QUAD of 4 consecutive pixels: 4 pixels x 3 bytes are exactly 3 dwords, 4 pixels x 4 bytes one
// 16-byte store, so no byte store is issued except in the last quad of an image whose pixel count is no multiple of 4 (narrow stores
// cost several times a dword store per byte on this part).  Plane c starts at float offset c P: when P is no multiple of 4, or a base
// pointer is not 16-byte aligned, that operand is read / written with dword accesses instead -- never a misaligned wide one.  The
// host decides that per operand (the `wide_*` bits), so the branch is uniform.
// Grid: 256 threads, min(quads / 256, TEXGS_PRESENT_MAX_WORKGROUPS) workgroups, grid-strided.
#include "common.h"
#include "abi_support.h"
#include "texgs_present.h"

#include <math.h>

namespace {

constexpr int PB = 256;
constexpr uint32_t PQ = TEXGS_PRESENT_PIXELS_PER_THREAD;
static_assert(PB * PQ == TEXGS_PRESENT_PIXELS_PER_WORKGROUP, "texgs_present.h states the pixels per workgroup");

// torch.clamp(v, 0, 1) by comparison: a NaN stays NaN, -0 stays -0
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// (uint8_t) trunc(v * 255): below 0 and NaN -> 0, 256 and above -> 255
__device__ __forceinline__ uint32_t quantise(float v) {
    const float t = v * 255.0f;
    return t > 0.f ? (t < 256.f ? (uint32_t)(int)t : 255u) : 0u;
}

// 4 consecutive floats at s (n of them exist): one 16-byte load when the host found the operand aligned, dwords otherwise
__device__ __forceinline__ void load_quad(const float* __restrict__ s, uint32_t n, bool wide, float (&v)[4]) {
    if (n == PQ && wide) {
        const float4 t = *reinterpret_cast<const float4*>(s);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < PQ; ++k) v[k] = k < n ? s[k] : 0.f;
    }
}

struct QuadOut {
    uint8_t* u8;
    float* hwc4;
    float* chw;
    uint32_t P;
    int u8_channels;
    int swap_rb;
    int wide_chw;
};

// One quad's outputs.  b[k][c]: the bytes of pixel k (r, g, b); f[k][c]: its floats.  p0 = 4 q is the quad's first pixel, n <= 4 exist.
__device__ __forceinline__ void emit_quad(const QuadOut& o, uint32_t p0, uint32_t n, const uint32_t (&b)[4][3], const float (&f)[4][3]) {
    if (o.u8) {
        uint32_t r[4], g[4], l[4];         // the bytes in stored order (selects, not indexed registers)
#pragma unroll
        for (uint32_t k = 0; k < PQ; ++k) { r[k] = o.swap_rb ? b[k][2] : b[k][0]; g[k] = b[k][1]; l[k] = o.swap_rb ? b[k][0] : b[k][2]; }
        if (n == PQ) {
            if (o.u8_channels == 3) {
                uint32_t* d = reinterpret_cast<uint32_t*>(o.u8 + (size_t)p0 * 3);
                d[0] = r[0] | (g[0] << 8) | (l[0] << 16) | (r[1] << 24);
                d[1] = g[1] | (l[1] << 8) | (r[2] << 16) | (g[2] << 24);
                d[2] = l[2] | (r[3] << 8) | (g[3] << 16) | (l[3] << 24);
            } else {
                uint4 w;
                w.x = r[0] | (g[0] << 8) | (l[0] << 16) | 0xFF000000u;
                w.y = r[1] | (g[1] << 8) | (l[1] << 16) | 0xFF000000u;
                w.z = r[2] | (g[2] << 8) | (l[2] << 16) | 0xFF000000u;
                w.w = r[3] | (g[3] << 8) | (l[3] << 16) | 0xFF000000u;
                *reinterpret_cast<uint4*>(o.u8 + (size_t)p0 * 4) = w;
            }
        } else {        // the image's last 1..3 pixels: bytes
            uint8_t* d = o.u8 + (size_t)p0 * o.u8_channels;
#pragma unroll
            for (uint32_t k = 0; k < PQ - 1; ++k) {
                if (k < n) {
                    d[0] = (uint8_t)r[k]; d[1] = (uint8_t)g[k]; d[2] = (uint8_t)l[k];
                    if (o.u8_channels == 4) d[3] = 255;
                    d += o.u8_channels;
                }
            }
        }
    }
    if (o.hwc4) {
        float4* d = reinterpret_cast<float4*>(o.hwc4) + p0;
#pragma unroll
        for (uint32_t k = 0; k < PQ; ++k)
            if (k < n) d[k] = make_float4(f[k][0], f[k][1], f[k][2], 1.0f);
    }
    if (o.chw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* d = o.chw + (size_t)c * o.P + p0;
            if (n == PQ && o.wide_chw) {
                *reinterpret_cast<float4*>(d) = make_float4(f[0][c], f[1][c], f[2][c], f[3][c]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < PQ; ++k)
                    if (k < n) d[k] = f[k][c];
            }
        }
    }
}

struct PresentArgs {
    const float* src;
    const float* alpha;
    const float* bg;
    QuadOut out;
    int channels;
    uint32_t flags;
    int wide_src;
    int wide_alpha;
};

__global__ void __launch_bounds__(PB)
k_present(PresentArgs a) {
    const uint32_t P = a.out.P, nq = (P + PQ - 1) / PQ;
    const bool affine = a.flags & TEXGS_PRESENT_AFFINE, composite = a.flags & TEXGS_PRESENT_COMPOSITE;
    float bg[3] = {0.f, 0.f, 0.f};
    if (composite && a.bg) { bg[0] = a.bg[0]; bg[1] = a.bg[1]; bg[2] = a.bg[2]; }
    for (uint32_t q = blockIdx.x * PB + threadIdx.x; q < nq; q += gridDim.x * PB) {
        const uint32_t p0 = q * PQ, n = P - p0 < PQ ? P - p0 : PQ;
        float v[3][4], al[4];
        load_quad(a.src + p0, n, a.wide_src, v[0]);
        if (a.channels == 3) {
            load_quad(a.src + (size_t)P + p0, n, a.wide_src, v[1]);
            load_quad(a.src + 2 * (size_t)P + p0, n, a.wide_src, v[2]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < PQ; ++k) v[1][k] = v[2][k] = v[0][k];
        }
        if (composite) load_quad(a.alpha + p0, n, a.wide_alpha, al);
        uint32_t b[4][3];
        float f[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (uint32_t k = 0; k < PQ; ++k) {
                float x = v[c][k];
                if (affine) x = 0.5f * (x + 1.0f);
                x = clamp01(x);
                if (composite) x = (x * al[k]) + (bg[c] * (1.0f - al[k]));
                f[k][c] = x;
                b[k][c] = quantise(x);
            }
        }
        emit_quad(a.out, p0, n, b, f);
    }
}

// ---- depth: range, then colour ----
// fminf / fmaxf: order-independent for the finite depths the contract asks for.  All 256 threads get the block's pair.
__device__ __forceinline__ void block_range(float& lo, float& hi, float* s_lo, float* s_hi) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m, 64));
        hi = fmaxf(hi, __shfl_xor(hi, m, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
}

__global__ void __launch_bounds__(PB)
k_depth_range(const float* __restrict__ depth, const float* __restrict__ mask, uint32_t P, int wide_depth, int wide_mask,
              float* __restrict__ parts /* [gridDim.x][2] */) {
    __shared__ float s_lo[4], s_hi[4];
    const uint32_t nq = (P + PQ - 1) / PQ;
    float lo = INFINITY, hi = -INFINITY;
    for (uint32_t q = blockIdx.x * PB + threadIdx.x; q < nq; q += gridDim.x * PB) {
        const uint32_t p0 = q * PQ, n = P - p0 < PQ ? P - p0 : PQ;
        float d[4], m[4];
        load_quad(depth + p0, n, wide_depth, d);
        if (mask) load_quad(mask + p0, n, wide_mask, m);
#pragma unroll
        for (uint32_t k = 0; k < PQ; ++k)
            if (k < n && (!mask || m[k] != 0.f)) { lo = fminf(lo, d[k]); hi = fmaxf(hi, d[k]); }
    }
    block_range(lo, hi, s_lo, s_hi);
    if (threadIdx.x == 0) { parts[2 * blockIdx.x] = lo; parts[2 * blockIdx.x + 1] = hi; }
}

struct DepthArgs {
    const float* depth;
    const float* mask;
    const uint8_t* lut;
    const float* parts;
    float* range;
    QuadOut out;
    int n_parts;
    int wide_depth;
    int wide_mask;
};

__global__ void __launch_bounds__(PB)
k_depth_colour(DepthArgs a) {
    __shared__ float s_lo[4], s_hi[4];
    __shared__ uint8_t s_lut[768];
    for (int i = threadIdx.x; i < 768; i += PB) s_lut[i] = a.lut[i];
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < a.n_parts; i += PB) { lo = fminf(lo, a.parts[2 * i]); hi = fmaxf(hi, a.parts[2 * i + 1]); }
    block_range(lo, hi, s_lo, s_hi);            // (its barrier also publishes s_lut)
    if (a.range && blockIdx.x == 0 && threadIdx.x == 0) { a.range[0] = lo; a.range[1] = hi; }
    const float den = (hi - lo) + 1e-8f;
    const uint32_t P = a.out.P, nq = (P + PQ - 1) / PQ;
    for (uint32_t q = blockIdx.x * PB + threadIdx.x; q < nq; q += gridDim.x * PB) {
        const uint32_t p0 = q * PQ, n = P - p0 < PQ ? P - p0 : PQ;
        float d[4], m[4];
        load_quad(a.depth + p0, n, a.wide_depth, d);
        if (a.mask) load_quad(a.mask + p0, n, a.wide_mask, m);
        uint32_t b[4][3];
        float f[4][3];
#pragma unroll
        for (uint32_t k = 0; k < PQ; ++k) {
            const float v = clamp01((d[k] - lo) / den);
            const float t = fabsf(v * 255.0f);
            const int idx = t >= 255.f ? 255 : (t > 0.f ? __float2int_rn(t) : 0);       // NaN -> 0
            const bool on = !a.mask || m[k] != 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                b[k][c] = on ? (uint32_t)s_lut[3 * idx + c] : 0u;
                f[k][c] = (float)b[k][c] / 255.0f;
            }
        }
        emit_quad(a.out, p0, n, b, f);
    }
}

// ---- cubemap cross ----
// The face of cell (row, column) of the 3 x 4 grid, one nibble per cell, 15 = empty (cube_map's placement)
constexpr unsigned long long CROSS_FACES = 0xFF3F5041FF2FULL;
constexpr float SH_C0 = 0.28209479177387814f;

__device__ __forceinline__ uint32_t cross_byte(float x) { return quantise(clamp01((x * SH_C0) + 0.5f)); }

// A quad of 4 output pixels is 12 bytes = 3 dwords; 12 R^2 pixels are always whole quads.  With R a multiple of 4 a quad lies in one
// cell and one row, and its 12 source floats are 48-byte aligned: three 16-byte loads.  Otherwise every pixel finds its own cell.
__global__ void __launch_bounds__(PB)
k_cube_cross(const float* __restrict__ tex, uint8_t* __restrict__ out, uint32_t R, int wide) {
    const uint32_t nq = 3u * R * R, W4 = 4u * R;
    for (uint32_t q = blockIdx.x * PB + threadIdx.x; q < nq; q += gridDim.x * PB) {
        const uint32_t p0 = q * 4u;
        uint32_t by[12];
        if (wide) {
            const uint32_t y = p0 / W4, x = p0 - y * W4, cy = y / R, cx = x / R;
            const uint32_t face = (uint32_t)(CROSS_FACES >> (4u * (cy * 4u + cx))) & 15u;
            if (face == 15u) {
#pragma unroll
                for (int i = 0; i < 12; ++i) by[i] = 0u;
            } else {
                const float4* s = reinterpret_cast<const float4*>(tex + ((size_t)(face * R + (y - cy * R)) * R + (x - cx * R)) * 3);
                const float4 t0 = s[0], t1 = s[1], t2 = s[2];
                by[0] = cross_byte(t0.x); by[1] = cross_byte(t0.y); by[2] = cross_byte(t0.z); by[3] = cross_byte(t0.w);
                by[4] = cross_byte(t1.x); by[5] = cross_byte(t1.y); by[6] = cross_byte(t1.z); by[7] = cross_byte(t1.w);
                by[8] = cross_byte(t2.x); by[9] = cross_byte(t2.y); by[10] = cross_byte(t2.z); by[11] = cross_byte(t2.w);
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t p = p0 + k, y = p / W4, x = p - y * W4, cy = y / R, cx = x / R;
                const uint32_t face = (uint32_t)(CROSS_FACES >> (4u * (cy * 4u + cx))) & 15u;
                if (face == 15u) {
                    by[3 * k] = by[3 * k + 1] = by[3 * k + 2] = 0u;
                } else {
                    const float* s = tex + ((size_t)(face * R + (y - cy * R)) * R + (x - cx * R)) * 3;
                    by[3 * k] = cross_byte(s[0]); by[3 * k + 1] = cross_byte(s[1]); by[3 * k + 2] = cross_byte(s[2]);
                }
            }
        }
        uint32_t* d = reinterpret_cast<uint32_t*>(out + (size_t)p0 * 3);
        d[0] = by[0] | (by[1] << 8) | (by[2] << 16) | (by[3] << 24);
        d[1] = by[4] | (by[5] << 8) | (by[6] << 16) | (by[7] << 24);
        d[2] = by[8] | (by[9] << 8) | (by[10] << 16) | (by[11] << 24);
    }
}

int quad_grid(uint32_t quads) {
    const uint32_t g = (quads + PB - 1) / PB;
    return (int)(g < TEXGS_PRESENT_MAX_WORKGROUPS ? g : TEXGS_PRESENT_MAX_WORKGROUPS);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

QuadOut quad_out(uint8_t* u8, float* hwc4, float* chw, uint32_t P, int u8_channels, uint32_t flags) {
    QuadOut o;
    o.u8 = u8; o.hwc4 = hwc4; o.chw = chw; o.P = P; o.u8_channels = u8_channels;
    o.swap_rb = (flags & TEXGS_PRESENT_SWAP_RB) ? 1 : 0;
    o.wide_chw = chw && P % PQ == 0 && aligned16(chw);
    return o;
}

}  // namespace

// (the arguments of the three launchers are validated by the entry points below)
static hipError_t launch_present(const TexGSPresent* p, hipStream_t s) {
    const uint32_t P = (uint32_t)p->height * (uint32_t)p->width;
    PresentArgs a;
    a.src = p->src; a.alpha = p->alpha; a.bg = p->background;
    a.out = quad_out(p->out_u8, p->out_hwc4, p->out_chw, P, p->u8_channels, p->flags);
    a.channels = p->channels; a.flags = p->flags;
    a.wide_src = aligned16(p->src) && (p->channels == 1 || P % PQ == 0);
    a.wide_alpha = p->alpha && aligned16(p->alpha);
    hipLaunchKernelGGL(k_present, dim3(quad_grid((P + PQ - 1) / PQ)), dim3(PB), 0, s, a);
    return hipGetLastError();
}

static size_t depth_colour_temp_bytes(int H, int W) {
    const uint32_t P = (uint32_t)H * (uint32_t)W;
    return (size_t)quad_grid((P + PQ - 1) / PQ) * 2 * sizeof(float);
}

static hipError_t launch_depth_colour(const TexGSDepthColour* d, void* temp, hipStream_t s) {
    const uint32_t P = (uint32_t)d->height * (uint32_t)d->width;
    const int grid = quad_grid((P + PQ - 1) / PQ);
    DepthArgs a;
    a.depth = d->depth; a.mask = d->mask; a.lut = d->lut; a.parts = (const float*)temp; a.range = d->range;
    a.out = quad_out(d->out_u8, d->out_hwc4, d->out_chw, P, d->u8_channels, d->flags);
    a.n_parts = grid;
    a.wide_depth = aligned16(d->depth);
    a.wide_mask = d->mask && aligned16(d->mask);
    hipLaunchKernelGGL(k_depth_range, dim3(grid), dim3(PB), 0, s, d->depth, d->mask, P, a.wide_depth, a.wide_mask, (float*)temp);
    hipLaunchKernelGGL(k_depth_colour, dim3(grid), dim3(PB), 0, s, a);
    return hipGetLastError();
}

static hipError_t launch_cube_cross(const TexGSCubeCross* c, hipStream_t s) {
    const uint32_t R = (uint32_t)c->res;
    const int wide = R % 4 == 0 && aligned16(c->texture);
    hipLaunchKernelGGL(k_cube_cross, dim3(quad_grid(3u * R * R)), dim3(PB), 0, s, c->texture, c->out, R, wide);
    return hipGetLastError();
}

extern "C" {

// include/texgs_present.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_present_image(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return fail_msg("height and width must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("image too large: height * width must be below 2^31");
    return 0;
}

static int check_present_outputs(const uint8_t* u8, int32_t u8_channels, const float* hwc4, const float* chw) {
    if (!u8 && !hwc4 && !chw) return fail_msg("no output requested (out_u8, out_hwc4 and out_chw are all NULL)");
    if (u8) {
        if (u8_channels != 3 && u8_channels != 4) return fail_msg("u8_channels must be 3 or 4");
        if ((uintptr_t)u8 & (u8_channels == 4 ? 15 : 3)) return fail_msg("out_u8 must be 4-byte aligned with 3 channels, 16-byte aligned with 4");
    }
    if ((uintptr_t)hwc4 & 15) return fail_msg("out_hwc4 must be 16-byte aligned");
    if ((uintptr_t)chw & 3) return fail_msg("out_chw must be 4-byte aligned");
    return 0;
}

int texgs_present(const TexGSPresent* p, void* stream) {
    if (!p) return fail_msg("present descriptor is NULL");
    if (int r = check_present_image(p->height, p->width)) return r;
    if (!p->src) return fail_msg("NULL argument (src)");
    if (p->channels != 1 && p->channels != 3) return fail_msg("channels must be 1 or 3");
    if (p->flags & ~(TEXGS_PRESENT_AFFINE | TEXGS_PRESENT_COMPOSITE | TEXGS_PRESENT_SWAP_RB)) return fail_msg("unknown bit in flags");
    if ((p->flags & TEXGS_PRESENT_COMPOSITE) && !p->alpha) return fail_msg("composite mode needs alpha");
    if (int r = check_present_outputs(p->out_u8, p->u8_channels, p->out_hwc4, p->out_chw)) return r;
    if (((uintptr_t)p->src | (uintptr_t)p->alpha | (uintptr_t)p->background) & 3) return fail_msg("src, alpha and background must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("present", launch_present(p, s), s, false);
}

size_t texgs_depth_colour_temp_bytes(int32_t height, int32_t width) {
    return check_present_image(height, width) ? 0 : depth_colour_temp_bytes(height, width);
}

int texgs_depth_colour(const TexGSDepthColour* d, void* temp, size_t temp_bytes, void* stream) {
    if (!d) return fail_msg("depth descriptor is NULL");
    if (int r = check_present_image(d->height, d->width)) return r;
    if (!d->depth || !d->lut || !temp) return fail_msg("NULL argument (depth, lut or temp)");
    if (d->flags & ~TEXGS_PRESENT_SWAP_RB) return fail_msg("unknown bit in flags (the depth picture reads TEXGS_PRESENT_SWAP_RB only)");
    if (int r = check_present_outputs(d->out_u8, d->u8_channels, d->out_hwc4, d->out_chw)) return r;
    if (((uintptr_t)d->depth | (uintptr_t)d->mask | (uintptr_t)d->range | (uintptr_t)temp) & 3)
        return fail_msg("depth, mask, range and temp must be 4-byte aligned");
    if (temp_bytes < depth_colour_temp_bytes(d->height, d->width)) return fail_msg("temp is smaller than texgs_depth_colour_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("depth_colour", launch_depth_colour(d, temp, s), s, false);
}

int texgs_cube_cross(const TexGSCubeCross* c, void* stream) {
    if (!c) return fail_msg("cross descriptor is NULL");
    if (c->res < 1 || c->res > 7168) return fail_msg("res must be in [1,7168]");
    if (!c->texture || !c->out) return fail_msg("NULL argument (texture or out)");
    if (((uintptr_t)c->texture | (uintptr_t)c->out) & 3) return fail_msg("texture and out must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_cross", launch_cube_cross(c, s), s, false);
}

}  // extern "C"
