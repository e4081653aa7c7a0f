// The backward of LPIPS-VGG in the images (include/texgs_lpips_grad.h): the streaming kernels between the data-gradient
// convolutions.  The convolutions themselves are k_conv3x3 of lpips.hip, unchanged, over transposed and flipped weights.
//
// HEAD BACKWARD  k_lpips_head_backward: one thread per pixel, pixels along the lanes, so every channel step of the walk is one
//   coalesced row segment per wave, as in k_lpips_head.  Three walks over the channels: the norms; t = sum_c r_c f_c, which needs the
//   norms; and the output, which needs t.  The third walk also finishes the layer's gradient -- the unpooled gradient of the next
//   slice and the ReLU gate -- so the gradient map is written exactly once and never read back.  The window's other three values come
//   from the lines that the neighbouring lanes and the neighbouring row's wave load anyway.
//   f32 with one rounding per operation (build.py: -ffp-contract=off): swapping the images negates r and t exactly, so the partner's
//   gradient of (a, b) is the first image's gradient of (b, a) bit for bit.  lin[c] and gbar[p] are wave-uniform (scalar loads).
// GATE  k_lpips_gate: 16 bytes per lane in a grid-stride loop; the n % 4 trailing elements go one per thread of the first block.
#include "common.h"
#include "lpips_checks.h"
#include "texgs_lpips.h"
#include "texgs_lpips_grad.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct HeadBwdArgs {
    const float* f;
    const float* lin;
    const float* gbar;
    const float* gn;             // [B', C, hn, wn] or nullptr
    float* G;
    long long gr, gc, gi;        // strides of G in floats: row, channel plane, image
    int P, C, h, w, hn, wn, wrt;
};

// whether (y, x) holds the FIRST maximum, in row-major order, of its 2x2 window of the plane q (row stride w)
__device__ __forceinline__ bool lp_first_max(const float* __restrict__ q, int w, int y, int x) {
    const float* __restrict__ b = q + (size_t)(y & ~1) * w + (x & ~1);
    const float v00 = b[0], v01 = b[1], v10 = b[w], v11 = b[w + 1];
    const float m = fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
    const int first = v00 == m ? 0 : v01 == m ? 1 : v10 == m ? 2 : 3;
    return first == (y & 1) * 2 + (x & 1);
}

__global__ void __launch_bounds__(256)
k_lpips_head_backward(HeadBwdArgs a) {
    const int p = blockIdx.y;
    const long long hw = (long long)a.h * a.w;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int y = (int)(pix / a.w), x = (int)(pix - (long long)y * a.w);
    const size_t img = (size_t)a.C * hw;
    const float* __restrict__ f0 = a.f + (size_t)p * img + pix;
    const float* __restrict__ f1 = a.f + (size_t)(a.P + p) * img + pix;

    // (unrolled: the sums stay in channel order, but the loads of eight channels are in flight together)
    float q0 = 0.0f, q1 = 0.0f;
#pragma unroll 8
    for (int c = 0; c < a.C; ++c) {
        const float u = f0[(size_t)c * hw], v = f1[(size_t)c * hw];
        q0 += u * u;
        q1 += v * v;
    }
    const float n0 = sqrtf(q0), n1 = sqrtf(q1);
    const float d0 = n0 + 1e-10f, d1 = n1 + 1e-10f;
    float t0 = 0.0f, t1 = 0.0f;
#pragma unroll 8
    for (int c = 0; c < a.C; ++c) {
        const float u = f0[(size_t)c * hw], v = f1[(size_t)c * hw];
        const float r = (2.0f * a.lin[c]) * (u / d0 - v / d1);
        t0 += r * u;
        t1 += r * v;
    }
    const float s = a.gbar[p] / (float)hw;
    const float k0 = t0 / (n0 * (d0 * d0)), k1 = (-t1) / (n1 * (d1 * d1));      // not finite at n = 0: selected away below

    const bool do0 = a.wrt & TEXGS_LPIPS_WRT_FIRST, do1 = a.wrt & TEXGS_LPIPS_WRT_PARTNER;
    const int slot1 = do0 ? a.P + p : p;                         // the partners follow the first images only when both are selected
    const bool window = a.gn != nullptr && (y >> 1) < a.hn && (x >> 1) < a.wn;
    const size_t hwn = (size_t)a.hn * a.wn, cell = window ? (size_t)(y >> 1) * a.wn + (x >> 1) : 0;
    const float* __restrict__ gn0 = a.gn + (size_t)p * a.C * hwn + cell;
    const float* __restrict__ gn1 = a.gn + (size_t)slot1 * a.C * hwn + cell;
    float* __restrict__ G0 = a.G + p * a.gi + y * a.gr + x;
    float* __restrict__ G1 = a.G + slot1 * a.gi + y * a.gr + x;
    const float* __restrict__ w0 = a.f + (size_t)p * img, * __restrict__ w1 = a.f + (size_t)(a.P + p) * img;
#pragma unroll 4
    for (int c = 0; c < a.C; ++c) {
        const float u = f0[(size_t)c * hw], v = f1[(size_t)c * hw];
        const float r = (2.0f * a.lin[c]) * (u / d0 - v / d1);
        if (do0) {
            float g = n0 > 0.0f ? s * (r / d0 - u * k0) : 0.0f;
            if (window && lp_first_max(w0 + (size_t)c * hw, a.w, y, x)) g = gn0[c * hwn] + g;
            G0[c * a.gc] = u > 0.0f ? g : 0.0f;
        }
        if (do1) {
            float g = n1 > 0.0f ? s * ((-r) / d1 - v * k1) : 0.0f;
            if (window && lp_first_max(w1 + (size_t)c * hw, a.w, y, x)) g = gn1[c * hwn] + g;
            G1[c * a.gc] = v > 0.0f ? g : 0.0f;
        }
    }
}

__global__ void __launch_bounds__(256)
k_lpips_gate(float* __restrict__ G, const float* __restrict__ y, long long nvec, long long n) {
    f32x4* __restrict__ G4 = reinterpret_cast<f32x4*>(G);
    const f32x4* __restrict__ y4 = reinterpret_cast<const f32x4*>(y);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long i = t; i < nvec; i += step) {
        f32x4 g = G4[i];
        const f32x4 v = y4[i];
        g.x = v.x > 0.0f ? g.x : 0.0f;
        g.y = v.y > 0.0f ? g.y : 0.0f;
        g.z = v.z > 0.0f ? g.z : 0.0f;
        g.w = v.w > 0.0f ? g.w : 0.0f;
        G4[i] = g;
    }
    const long long e = 4 * nvec + t;                            // the tail: at most three elements, one thread each
    if (e < n) G[e] = y[e] > 0.0f ? G[e] : 0.0f;
}

constexpr int LP_GATE_MAX_BLOCKS = 4096;

}  // namespace

static hipError_t launch_lpips_head_backward(const TexGSLpipsHeadBackward* d, hipStream_t s) {
    const long long hw = (long long)d->h * d->w;
    const bool dense = !d->g_row && !d->g_chan && !d->g_img;
    const long long gr = dense ? d->w : d->g_row, gc = dense ? gr * d->h : d->g_chan, gi = dense ? gc * d->C : d->g_img;
    const HeadBwdArgs a{d->f, d->lin, d->gbar, d->g_next, d->G, gr, gc, gi, d->P, d->C, d->h, d->w, d->h / 2, d->w / 2, d->wrt};
    hipLaunchKernelGGL(k_lpips_head_backward, dim3((unsigned)((hw + 255) / 256), d->P), dim3(256), 0, s, a);
    return hipGetLastError();
}

static hipError_t launch_lpips_gate(float* G, const float* y, long long n, hipStream_t s) {
    const long long nvec = n / 4, blocks = (nvec + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1 ? 1 : blocks > LP_GATE_MAX_BLOCKS ? LP_GATE_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(k_lpips_gate, dim3(grid), dim3(256), 0, s, G, y, nvec, n);
    return hipGetLastError();
}

extern "C" {

// include/texgs_lpips_grad.h: every argument is checked before the launch, so a refused call has changed nothing
int texgs_lpips_head_backward(const TexGSLpipsHeadBackward* d, void* stream) {
    if (!d) return fail_msg("head backward descriptor is NULL");
    if (int r = check_lpips_head_size(d->P, d->h, d->w)) return r;
    if (d->C < 1 || d->C > TEXGS_CONV_MAX_CHANNELS) return failf("C must be in [1,512], got %d", (int)d->C);
    if (d->wrt < 1 || d->wrt > (TEXGS_LPIPS_WRT_FIRST | TEXGS_LPIPS_WRT_PARTNER))
        return failf("wrt must be 1 (first images), 2 (partners) or 3 (both), got %d", (int)d->wrt);
    if (d->g_next && (d->h < 2 || d->w < 2)) return fail_msg("g_next needs h and w of at least 2: the pooled map would be empty");
    const int64_t Bg = d->wrt == 3 ? 2 * (int64_t)d->P : d->P;
    if (int r = check_conv_strides("g", d->g_row, d->g_chan, d->g_img, Bg, d->C, d->h, d->w)) return r;
    if (!d->f || !d->lin || !d->gbar || !d->G) return fail_msg("NULL argument (f, lin, gbar or G)");
    if (((uintptr_t)d->f | (uintptr_t)d->lin | (uintptr_t)d->gbar | (uintptr_t)d->g_next | (uintptr_t)d->G) & 3)
        return fail_msg("f, lin, gbar, g_next and G must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("lpips_head_backward", launch_lpips_head_backward(d, s), s, false);
}

int texgs_lpips_gate(float* G, const float* y, int64_t n, void* stream) {
    if (n < 1 || n >= (1ll << 40)) return failf("n must be in [1,2^40), got %lld", (long long)n);
    if (!G || !y) return fail_msg("NULL argument (G or y)");
    if (((uintptr_t)G | (uintptr_t)y) & 15) return fail_msg("G and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("lpips_gate", launch_lpips_gate(G, y, n, s), s, false);
}

}  // extern "C"
