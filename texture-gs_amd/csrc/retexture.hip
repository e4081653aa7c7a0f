// The retexture stage (include/texgs_retexture.h): a picture -- the 8-bit cubemap cross or a lat-long map -- into the SH-DC texture,
// with change_texture's mode arithmetic, as ONE streaming pass over the texture each.  Built with -ffp-contract=off: the per-texel
// arithmetic (retexture_math.h) is compared bit for bit with tests/retexture_ref.py.
//
// The texture is walked as a flat array of 6 R^2 texels of 12 bytes; every texel decodes its own face, row and column.  The cross
// kernel gives a thread TPT consecutive texels.  TPT = 1, the mapping that is built (TEXGS_RETEX_TEXELS_PER_THREAD), is 12 bytes per
// lane as three dwords.  TPT = 4 is the other mapping the kernel was measured with (an experiment build with
// -DTEXGS_RETEX_BUILD_TPT=4): 48 bytes per thread, a multiple of 16 wherever the group starts, moved as three 16-byte accesses when
// both pointers are 16-byte aligned, with dwords for the last group of the array (6 R^2 is 2 modulo 4 when R is odd).  It was
// SLOWER on the MI355X, 56 against 48 us at R = 1024 and 250 against 200 us at R = 2048 (profiles/retexture_kernel_stats.csv): the
// kernel runs at half the copy bandwidth and is bound by its fp64 blend and the latency of the byte taps, not by the width of
// the texture accesses, and a quarter of the threads hide that latency worse.  The source pixels under a texel's taps are read as
// bytes, through the caches: neighbouring texels share them.  No LDS, no atomics.
// In place (out_tex == old_tex) is safe: a thread loads its own old texels before it stores them, and nobody else reads them.
#include "common.h"
#include "abi_support.h"
#include "texgs_retexture.h"
#include "retexture_math.h"

namespace {

namespace rm = retexture_math;
constexpr int RT = TEXGS_RETEX_THREADS;

#ifndef TEXGS_RETEX_BUILD_TPT           // experiment builds: the other texel-to-lane mapping
#define TEXGS_RETEX_BUILD_TPT TEXGS_RETEX_TEXELS_PER_THREAD
#endif
constexpr int TPT = TEXGS_RETEX_BUILD_TPT;
static_assert(TPT == 1 || TPT == 4, "one texel per lane, or four (three 16-byte accesses)");

struct Texel {
    uint32_t f, y, x;
};

__device__ __forceinline__ Texel texel_of(uint32_t t, uint32_t R) {
    const uint32_t row = t / R;          // f R + y
    Texel p;
    p.x = t - row * R;
    p.f = row / R;
    p.y = row - p.f * R;
    return p;
}

__device__ __forceinline__ void next_texel(Texel& p, uint32_t R) {
    if (++p.x == R) {
        p.x = 0;
        if (++p.y == R) {
            p.y = 0;
            ++p.f;
        }
    }
}

// K consecutive texels from global memory into v (3 K floats) and back; wide: 16-byte accesses (K == 4, pointer 16-byte aligned)
template <int K>
__device__ __forceinline__ void load_texels(const float* p, float* v, int count, bool wide) {
    if (K == 4 && wide) {
        const float4* q = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 a = q[k];
            v[4 * k] = a.x; v[4 * k + 1] = a.y; v[4 * k + 2] = a.z; v[4 * k + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * K; ++k)
            if (k < 3 * count) v[k] = p[k];
    }
}

template <int K>
__device__ __forceinline__ void store_texels(float* p, const float* v, int count, bool wide) {
    if (K == 4 && wide) {
        float4* q = reinterpret_cast<float4*>(p);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * K; ++k)
            if (k < 3 * count) p[k] = v[k];
    }
}

// sx = 4r / 4R and sy = 3r / 3R as the host divides them (fp64); total = 6 R^2 < 2^31; aligned16: old_tex and out_tex both are
template <int K>
__global__ void __launch_bounds__(RT)
k_retexture_cross(TexGSRetexCross c, double sx, double sy, uint32_t total, int aligned16) {
    const uint64_t g = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (g * K >= total) return;
    const uint32_t t0 = (uint32_t)(g * K);
    const int count = total - t0 < (uint32_t)K ? (int)(total - t0) : K;
    const bool wide = aligned16 && count == K;
    const uint32_t R = (uint32_t)c.R;
    const int32_t in_h = 3 * c.r, in_w = 4 * c.r;
    const size_t at = 3 * (size_t)t0;

    float v[3 * K];
#pragma unroll
    for (int k = 0; k < 3 * K; ++k) v[k] = 0.0f;
    if (c.mode != -1) load_texels<K>(c.old_tex + at, v, count, wide);

    Texel p = texel_of(t0, R);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k < count) {
            const rm::Tap ty = rm::cross_tap((int32_t)(rm::cross_row((int)p.f) * R + p.y), in_h, sy);
            const rm::Tap tx = rm::cross_tap((int32_t)(rm::cross_col((int)p.f) * R + p.x), in_w, sx);
            const uint8_t* r0 = c.src + 3 * ((size_t)ty.i0 * (size_t)in_w);
            const uint8_t* r1 = c.src + 3 * ((size_t)ty.i1 * (size_t)in_w);
            const size_t x0 = 3 * (size_t)tx.i0, x1 = 3 * (size_t)tx.i1;
            float n[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int sc = c.order == TEXGS_RETEX_BGR ? 2 - ch : ch;
                n[ch] = rm::unit_of_byte(rm::cross_blend(r0[x0 + sc], r0[x1 + sc], r1[x0 + sc], r1[x1 + sc], tx.w, ty.w));
            }
            rm::mode_tail(&v[3 * k], n, c.mode, &v[3 * k]);
            next_texel(p, R);
        }
    }
    store_texels<K>(c.out_tex + at, v, count, wide);
}

// one thread per texel
__global__ void __launch_bounds__(RT)
k_retexture_latlong(TexGSRetexLatLong l, uint32_t total) {
    const uint64_t t = (uint64_t)blockIdx.x * RT + threadIdx.x;
    if (t >= total) return;
    const Texel p = texel_of((uint32_t)t, (uint32_t)l.R);
    rm::Wrap tx, ty;
    rm::latlong_address((int)p.f, (int32_t)p.y, (int32_t)p.x, l.R, l.h, l.w, &tx, &ty);
    const size_t r0 = 3 * ((size_t)ty.i0 * (size_t)l.w), r1 = 3 * ((size_t)ty.i1 * (size_t)l.w);
    const size_t x0 = 3 * (size_t)tx.i0, x1 = 3 * (size_t)tx.i1;
    float n[3];
    if (l.src_u8) {
        const uint8_t* s = (const uint8_t*)l.src;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            n[ch] = rm::latlong_blend(rm::unit_of_byte(s[r0 + x0 + ch]), rm::unit_of_byte(s[r0 + x1 + ch]), rm::unit_of_byte(s[r1 + x0 + ch]),
                                      rm::unit_of_byte(s[r1 + x1 + ch]), tx.w, ty.w);
    } else {
        const float* s = (const float*)l.src;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            n[ch] = rm::latlong_blend(s[r0 + x0 + ch], s[r0 + x1 + ch], s[r1 + x0 + ch], s[r1 + x1 + ch], tx.w, ty.w);
    }
    const size_t at = 3 * (size_t)t;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (l.mode != -1) {
        v[0] = l.old_tex[at]; v[1] = l.old_tex[at + 1]; v[2] = l.old_tex[at + 2];
    }
    rm::mode_tail(v, n, l.mode, v);
    l.out_tex[at] = v[0]; l.out_tex[at + 1] = v[1]; l.out_tex[at + 2] = v[2];
}

inline uint32_t texels(int32_t R) { return 6u * (uint32_t)R * (uint32_t)R; }       // R <= 7168: 308 281 344

}  // namespace

static hipError_t launch_retexture_cross(const TexGSRetexCross* c, hipStream_t s) {
    const uint32_t total = texels(c->R);
    const uint32_t groups = (total + TPT - 1) / TPT;
    const int aligned16 = (((uintptr_t)c->old_tex | (uintptr_t)c->out_tex) & 15) == 0;
    const double sx = (double)(4 * c->r) / (double)(4 * c->R), sy = (double)(3 * c->r) / (double)(3 * c->R);
    hipLaunchKernelGGL(k_retexture_cross<TPT>, dim3((groups + RT - 1) / RT), dim3(RT), 0, s, *c, sx, sy, total, aligned16);
    return hipGetLastError();
}

static hipError_t launch_retexture_latlong(const TexGSRetexLatLong* l, hipStream_t s) {
    const uint32_t total = texels(l->R);
    hipLaunchKernelGGL(k_retexture_latlong, dim3((total + RT - 1) / RT), dim3(RT), 0, s, *l, total);
    return hipGetLastError();
}

extern "C" {

// include/texgs_retexture.h: every argument is checked before the launch, so a refused call has changed nothing
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

static int check_retexture(const void* src, size_t src_bytes, const float* old_tex, float* out_tex, int32_t R, int32_t mode) {
    if (R < 1 || R > TEXGS_RETEX_MAX_RES) return fail_msg("R must be in [1,7168]");
    if (mode < -1 || mode > 3) return fail_msg("mode must be -1, 0, 1, 2 or 3");
    if (!src) return fail_msg("NULL argument (src)");
    if (!out_tex) return fail_msg("NULL argument (out_tex)");
    if (!old_tex && mode != -1) return fail_msg("NULL argument (old_tex): only mode -1 does without the old texture");
    if (((uintptr_t)old_tex | (uintptr_t)out_tex) & 3) return fail_msg("old_tex and out_tex must be 4-byte aligned");
    const size_t tex_bytes = 6 * (size_t)R * (size_t)R * 3 * sizeof(float);
    if (old_tex && old_tex != out_tex && ranges_overlap(old_tex, tex_bytes, out_tex, tex_bytes))
        return fail_msg("out_tex overlaps old_tex without being equal to it (in place means the same pointer)");
    if (ranges_overlap(src, src_bytes, out_tex, tex_bytes)) return fail_msg("out_tex overlaps src");
    return 0;
}

int texgs_retexture_cross(const TexGSRetexCross* c, void* stream) {
    if (!c) return fail_msg("retexture cross descriptor is NULL");
    if (c->r < 1 || c->r > TEXGS_RETEX_MAX_SRC) return fail_msg("r must be in [1,16384]");
    if (c->order != TEXGS_RETEX_RGB && c->order != TEXGS_RETEX_BGR) return fail_msg("order must be 0 (rgb) or 1 (bgr)");
    if (int rc = check_retexture(c->src, 36 * (size_t)c->r * (size_t)c->r, c->old_tex, c->out_tex, c->R, c->mode)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return launched("retexture_cross", launch_retexture_cross(c, s), s, false);
}

int texgs_retexture_latlong(const TexGSRetexLatLong* l, void* stream) {
    if (!l) return fail_msg("retexture latlong descriptor is NULL");
    if (l->h < 1 || l->h > TEXGS_RETEX_MAX_SRC || l->w < 1 || l->w > TEXGS_RETEX_MAX_SRC) return fail_msg("h and w must be in [1,16384]");
    if (l->src_u8 != 0 && l->src_u8 != 1) return fail_msg("src_u8 must be 0 or 1");
    if (!l->src_u8 && ((uintptr_t)l->src & 3)) return fail_msg("a float src must be 4-byte aligned");
    const size_t src_bytes = 3 * (size_t)l->h * (size_t)l->w * (l->src_u8 ? 1 : sizeof(float));
    if (int rc = check_retexture(l->src, src_bytes, l->old_tex, l->out_tex, l->R, l->mode)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return launched("retexture_latlong", launch_retexture_latlong(l, s), s, false);
}

}  // extern "C"
