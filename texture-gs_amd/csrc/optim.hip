// Fused multi-tensor Adam step (include/texgs_optim.h): what three torch.optim.Adam(..., eps=1e-15).step() calls and a zero_grad of the
// reference's optimize_step (models/texture_gaussian3d.py:420-444) do, in one pass over p, g, m, v: 28 bytes per element moved
// (32 with zero_grads).  Built with -ffp-contract=off: the arithmetic is a bit-exact contract, one rounding per operation in the
// order written in adam_element (sqrtf and '/' are the correctly rounded ones here, denormals are kept).  No atomics, no LDS, every
// address is written by one lane.
//
// Up to TEXGS_ADAM_MAX_TENSORS records travel BY VALUE in the kernel arguments, with the prefix of their chunk counts: nothing is
// copied to the device, nothing allocated, nothing waited for.  Work is cut into chunks of TEXGS_ADAM_CHUNK elements over all the
// tensors of a launch; a workgroup finds the tensor of its chunk from the prefix and grid-strides over the chunks.
#include "common.h"
#include "abi_support.h"
#include "texgs_optim.h"

namespace {

constexpr int AD_BLOCK = 256;
constexpr int AD_VEC = 4;                               // floats of one 16-byte access
constexpr int AD_CHUNK = TEXGS_ADAM_CHUNK;              // one 16-byte access per lane and tensor
constexpr int AD_MAX = TEXGS_ADAM_MAX_TENSORS;
constexpr uint32_t AD_GRID_CAP = 2048;                  // 256 CUs x 8 workgroups; the rest is grid-strided
static_assert(AD_CHUNK == AD_BLOCK * AD_VEC, "a chunk is one 16-byte access per lane");
static_assert(sizeof(TexGSAdamTensor) == 64, "the record is 64 bytes");

struct AdamArgs {
    TexGSAdamTensor t[AD_MAX];
    uint64_t first_chunk[AD_MAX + 1];       // chunks [first_chunk[k], first_chunk[k+1]) belong to t[k]; empty for numel == 0
    int32_t count;
    int32_t zero_grads;
};

struct AdamScalars {
    float w1, one_minus_w1, beta2, w2, bc2_sqrt, eps, neg_step_size;
    bool low;                               // w1 < 0.5: which side torch's lerp interpolates from
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamScalars& s) {
    const float d = g - m;
    const float m1 = s.low ? m + s.w1 * d : g - d * s.one_minus_w1;
    float v1 = v * s.beta2;
    v1 = v1 + (s.w2 * g) * g;
    const float den = sqrtf(v1) / s.bc2_sqrt + s.eps;
    p = p + s.neg_step_size * (m1 / den);
    m = m1;
    v = v1;
}

__global__ void __launch_bounds__(AD_BLOCK)
k_adam_step(AdamArgs a) {
    const uint64_t total = a.first_chunk[a.count];
    int t = 0;
    for (uint64_t c = blockIdx.x; c < total; c += gridDim.x) {
        while (c >= a.first_chunk[t + 1]) ++t;          // c only grows; t + 1 <= count because c < first_chunk[count]
        const TexGSAdamTensor R = a.t[t];
        const int64_t e0 = (int64_t)(c - a.first_chunk[t]) * AD_CHUNK;
        const int64_t left = R.numel - e0;
        const int n = left < AD_CHUNK ? (int)left : AD_CHUNK;
        float* __restrict__ p = R.p + e0;
        float* __restrict__ g = R.g + e0;
        float* __restrict__ m = R.m + e0;
        float* __restrict__ v = R.v + e0;
        AdamScalars s;
        s.w1 = R.w1; s.one_minus_w1 = 1.0f - R.w1; s.beta2 = R.beta2; s.w2 = R.w2; s.bc2_sqrt = R.bc2_sqrt; s.eps = R.eps;
        s.neg_step_size = R.neg_step_size; s.low = R.w1 < 0.5f;
        // e0 is a multiple of 4 elements, so a chunk's pointers are aligned like the tensor's
        const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
        const int i = (int)threadIdx.x * AD_VEC;
        if (aligned && i + AD_VEC <= n) {
            float4 P = *reinterpret_cast<const float4*>(p + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            float4 M = *reinterpret_cast<const float4*>(m + i);
            float4 V = *reinterpret_cast<const float4*>(v + i);
            adam_element(P.x, G.x, M.x, V.x, s);
            adam_element(P.y, G.y, M.y, V.y, s);
            adam_element(P.z, G.z, M.z, V.z, s);
            adam_element(P.w, G.w, M.w, V.w, s);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
            if (a.zero_grads) *reinterpret_cast<float4*>(g + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else if (aligned) {                           // the tensor's last, partial group of four
            for (int j = i; j < n; ++j) {
                float P = p[j], M = m[j], V = v[j];
                adam_element(P, g[j], M, V, s);
                p[j] = P; m[j] = M; v[j] = V;
                if (a.zero_grads) g[j] = 0.0f;
            }
        } else {                                        // some pointer is off a 16-byte boundary: consecutive lanes, 4-byte accesses
            for (int j = (int)threadIdx.x; j < n; j += AD_BLOCK) {
                float P = p[j], M = m[j], V = v[j];
                adam_element(P, g[j], M, V, s);
                p[j] = P; m[j] = M; v[j] = V;
                if (a.zero_grads) g[j] = 0.0f;
            }
        }
    }
}

}  // namespace

// One launch over `count` <= TEXGS_ADAM_MAX_TENSORS records (texgs_adam_step below cuts longer lists)
static hipError_t launch_adam_step(const TexGSAdamTensor* tensors, int count, int zero_grads, hipStream_t s) {
    if (count < 0 || count > AD_MAX) return hipErrorInvalidValue;
    AdamArgs a;
    uint64_t chunks = 0;
    for (int k = 0; k < count; ++k) {
        a.t[k] = tensors[k];
        a.first_chunk[k] = chunks;
        chunks += ((uint64_t)tensors[k].numel + AD_CHUNK - 1) / AD_CHUNK;
    }
    for (int k = count; k <= AD_MAX; ++k) a.first_chunk[k] = chunks;
    for (int k = count; k < AD_MAX; ++k) a.t[k] = TexGSAdamTensor{nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f};
    a.count = count;
    a.zero_grads = zero_grads != 0;
    if (chunks == 0) return hipSuccess;
    const uint32_t grid = chunks < AD_GRID_CAP ? (uint32_t)chunks : AD_GRID_CAP;
    hipLaunchKernelGGL(k_adam_step, dim3(grid), dim3(AD_BLOCK), 0, s, a);
    return hipGetLastError();
}

// include/texgs_optim.h: every record is checked before the first launch, so a refused call has changed nothing
extern "C" int texgs_adam_step(const TexGSAdamTensor* tensors, int32_t count, int32_t zero_grads, void* stream) {
    if (count < 0) return fail_msg("count < 0");
    if (count == 0) return 0;
    if (!tensors) return fail_msg("tensors is NULL");
    for (int32_t k = 0; k < count; ++k) {
        const TexGSAdamTensor& t = tensors[k];
        if (t.numel < 0) return fail_msg("numel < 0");
        if (t.numel == 0) continue;
        if (!t.p || !t.g || !t.m || !t.v) return fail_msg("NULL pointer (p, g, m or v) in a record with numel > 0");
        if (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3)
            return fail_msg("p, g, m and v must be 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    for (int32_t first = 0; first < count; first += TEXGS_ADAM_MAX_TENSORS) {
        const int32_t n = count - first < TEXGS_ADAM_MAX_TENSORS ? count - first : TEXGS_ADAM_MAX_TENSORS;
        if (int r = launched("adam_step", launch_adam_step(tensors + first, n, zero_grads, s), s, false)) return r;
    }
    return 0;
}
