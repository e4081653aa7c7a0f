// The parameter stage (include/texgs_params.h): stored parameters -> the operator's inputs (exp, F.normalize, sigmoid), the opacity
// regulariser, get_covariance, and their backwards -- what the reference runs as a chain of small torch launches on every render.
// Built with -ffp-contract=off: the row arithmetic (params_math.h) is compared bit for bit with tests/params_ref.py, and a row's
// result must not depend on n or on the row's position.
//
// One thread per row, PB rows per workgroup, the grid covers n rows: 32 bytes in and 32 bytes out per row.
//   * the quaternion moves as one 16-byte access per lane;
//   * opacity is one dword per lane, consecutive across the wave;
//   * scaling is elementwise in the activation and its backward, so a workgroup walks its 3 PB floats as three dense passes
//     (lane t takes elements t, t + PB, t + 2 PB); the covariance needs a row's three together and stages them through LDS the
//     same way, as it does its six outputs, so global memory sees dense dwords only.
// The regulariser's sum is fp64 in a fixed order: a tree over the workgroup's rows, then one workgroup over the partials.
#include "common.h"
#include "abi_support.h"
#include "texgs_params.h"
#include "params_math.h"

namespace {

namespace pm = params_math;
constexpr int PB = TEXGS_PARAMS_ROWS_PER_WORKGROUP;
static_assert(PB == 256 && (PB & (PB - 1)) == 0, "the tree below halves PB down to one");

// the workgroup's sum of v over its PB threads, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s) {
    s[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int d = PB / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    return s[0];
}

// K floats per row of the workgroup's `rows` rows (from row0 on), between global memory and LDS as dense dwords
template <int K>
__device__ __forceinline__ void stage_in(const float* __restrict__ src, float* lds, size_t row0, uint32_t rows) {
    const float* base = src + (size_t)K * row0;
    for (uint32_t i = threadIdx.x; i < K * rows; i += PB) lds[i] = base[i];
}

template <int K>
__device__ __forceinline__ void stage_out(float* __restrict__ dst, const float* lds, size_t row0, uint32_t rows) {
    float* base = dst + (size_t)K * row0;
    for (uint32_t i = threadIdx.x; i < K * rows; i += PB) base[i] = lds[i];
}

__device__ __forceinline__ void load_quat(const float* __restrict__ p, size_t row, float q[4]) {
    const float4 v = reinterpret_cast<const float4*>(p)[row];
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
}

__device__ __forceinline__ void store_quat(float* __restrict__ p, size_t row, const float q[4]) {
    reinterpret_cast<float4*>(p)[row] = make_float4(q[0], q[1], q[2], q[3]);
}

__global__ void __launch_bounds__(PB)
k_params_activate(TexGSParamsActivate a, double* __restrict__ partials) {
    __shared__ double s_sum[PB];
    const uint32_t n = (uint32_t)a.n;
    const size_t row0 = (size_t)blockIdx.x * PB;
    const size_t i = row0 + threadIdx.x;
    if (a.scales) {
        const size_t end = 3 * (size_t)n;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t e = 3 * row0 + threadIdx.x + (size_t)j * PB;
            if (e < end) a.scales[e] = pm::exp32(a.scaling[e]);
        }
    }
    if (a.rotations && i < n) {
        float q[4], r[4];
        load_quat(a.rotation, i, q);
        pm::normalize(q, r);
        store_quat(a.rotations, i, r);
    }
    if (a.opacities || a.reg) {
        double term = 0.0;
        if (i < n) {
            const float o = pm::sigmoid32(a.opacity[i]);
            if (a.opacities) a.opacities[i] = o;
            if (a.reg) term = (double)pm::reg_term(o, a.epsilon);
        }
        if (a.reg) {            // (uniform: a kernel argument)
            const double sum = block_sum(term, s_sum);
            if (threadIdx.x == 0) partials[blockIdx.x] = sum;
        }
    }
}

// one workgroup: thread j adds partials j, j + PB, ... in that order, then the tree
__global__ void __launch_bounds__(PB)
k_params_reg_finish(const double* __restrict__ partials, uint32_t count, uint32_t n, float* __restrict__ reg) {
    __shared__ double s_sum[PB];
    double acc = 0.0;
    for (uint32_t j = threadIdx.x; j < count; j += PB) acc += partials[j];
    const double sum = block_sum(acc, s_sum);
    if (threadIdx.x == 0) *reg = (float)(sum / (double)n);
}

__global__ void __launch_bounds__(PB)
k_params_activate_backward(TexGSParamsActivateGrad g) {
    const uint32_t n = (uint32_t)g.n;
    const size_t row0 = (size_t)blockIdx.x * PB;
    const size_t i = row0 + threadIdx.x;
    if (g.d_scaling) {
        const size_t end = 3 * (size_t)n;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const size_t e = 3 * row0 + threadIdx.x + (size_t)j * PB;
            if (e < end) g.d_scaling[e] = g.g_scales ? g.g_scales[e] * g.scales[e] : 0.0f;
        }
    }
    if (i >= n) return;
    if (g.d_rotation) {
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (g.g_rotations) {
            float q[4], u[4];
            load_quat(g.rotation, i, q);
            load_quat(g.g_rotations, i, u);
            pm::normalize_backward(q, u, d);
        }
        store_quat(g.d_rotation, i, d);
    }
    if (g.d_opacity) {
        float d = 0.0f;
        if (g.g_opacities || g.g_reg) {
            const float c = g.g_reg ? *g.g_reg / (float)n : 0.0f;
            d = pm::opacity_backward(g.opacities[i], g.g_opacities ? g.g_opacities[i] : 0.0f, g.g_reg != nullptr, c, g.epsilon);
        }
        g.d_opacity[i] = d;
    }
}

__global__ void __launch_bounds__(PB)
k_params_covariance(TexGSParamsCovariance c) {
    __shared__ float s_a[3 * PB];
    __shared__ float s_cov[6 * PB];
    const uint32_t n = (uint32_t)c.n;
    const size_t row0 = (size_t)blockIdx.x * PB;
    const uint32_t rows = n - row0 < (size_t)PB ? (uint32_t)(n - row0) : (uint32_t)PB;
    stage_in<3>(c.scaling, s_a, row0, rows);
    __syncthreads();
    if (threadIdx.x < rows) {
        float q[4], cov[6];
        const float a[3] = {s_a[3 * threadIdx.x], s_a[3 * threadIdx.x + 1], s_a[3 * threadIdx.x + 2]};
        load_quat(c.rotation, row0 + threadIdx.x, q);
        pm::covariance(a, q, c.scale_modifier, cov);
#pragma unroll
        for (int k = 0; k < 6; ++k) s_cov[6 * threadIdx.x + k] = cov[k];
    }
    __syncthreads();
    stage_out<6>(c.cov, s_cov, row0, rows);
}

__global__ void __launch_bounds__(PB)
k_params_covariance_backward(TexGSParamsCovarianceGrad c) {
    __shared__ float s_a[3 * PB];            // scaling in, d_scaling out
    __shared__ float s_g[6 * PB];
    const uint32_t n = (uint32_t)c.n;
    const size_t row0 = (size_t)blockIdx.x * PB;
    const uint32_t rows = n - row0 < (size_t)PB ? (uint32_t)(n - row0) : (uint32_t)PB;
    stage_in<3>(c.scaling, s_a, row0, rows);
    if (c.g_cov) stage_in<6>(c.g_cov, s_g, row0, rows);
    __syncthreads();
    if (threadIdx.x < rows) {
        float q[4], g[6], da[3], dq[4];
        const float a[3] = {s_a[3 * threadIdx.x], s_a[3 * threadIdx.x + 1], s_a[3 * threadIdx.x + 2]};
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = c.g_cov ? s_g[6 * threadIdx.x + k] : 0.0f;
        load_quat(c.rotation, row0 + threadIdx.x, q);
        if (c.g_cov) {
            pm::covariance_backward(a, q, c.scale_modifier, g, da, dq);
        } else {                // a zero gradient is zero, also where the row is not finite
            da[0] = da[1] = da[2] = 0.0f;
            dq[0] = dq[1] = dq[2] = dq[3] = 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) s_a[3 * threadIdx.x + k] = da[k];       // the thread's own three: read above, by it alone
        if (c.d_rotation) store_quat(c.d_rotation, row0 + threadIdx.x, dq);
    }
    __syncthreads();
    if (c.d_scaling) stage_out<3>(c.d_scaling, s_a, row0, rows);
}

inline uint32_t params_groups(int32_t n) { return ((uint32_t)n + PB - 1) / PB; }

}  // namespace

static size_t params_temp_bytes(int32_t n) { return ((size_t)params_groups(n) * sizeof(double) + 255) & ~(size_t)255; }

static hipError_t launch_params_activate(const TexGSParamsActivate* a, void* temp, hipStream_t s) {
    const uint32_t groups = params_groups(a->n);
    hipLaunchKernelGGL(k_params_activate, dim3(groups), dim3(PB), 0, s, *a, (double*)temp);
    if (a->reg) hipLaunchKernelGGL(k_params_reg_finish, dim3(1), dim3(PB), 0, s, (const double*)temp, groups, (uint32_t)a->n, a->reg);
    return hipGetLastError();
}

static hipError_t launch_params_activate_backward(const TexGSParamsActivateGrad* g, hipStream_t s) {
    hipLaunchKernelGGL(k_params_activate_backward, dim3(params_groups(g->n)), dim3(PB), 0, s, *g);
    return hipGetLastError();
}

static hipError_t launch_params_covariance(const TexGSParamsCovariance* c, hipStream_t s) {
    hipLaunchKernelGGL(k_params_covariance, dim3(params_groups(c->n)), dim3(PB), 0, s, *c);
    return hipGetLastError();
}

static hipError_t launch_params_covariance_backward(const TexGSParamsCovarianceGrad* c, hipStream_t s) {
    hipLaunchKernelGGL(k_params_covariance_backward, dim3(params_groups(c->n)), dim3(PB), 0, s, *c);
    return hipGetLastError();
}

extern "C" {

// include/texgs_params.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_params_epsilon(float e) {
    if (!(e > 0.0f && e < 0.5f)) return fail_msg("epsilon must lie in (0, 0.5)");
    return 0;
}

static int check_params_modifier(float m) {
    if (!(m > 0.0f) || m - m != 0.0f) return fail_msg("scale_modifier must be finite and positive");
    return 0;
}

size_t texgs_params_temp_bytes(int32_t n) { return n <= 0 ? 0 : params_temp_bytes(n); }

int texgs_params_activate(const TexGSParamsActivate* a, void* temp, size_t temp_bytes, void* stream) {
    if (!a) return fail_msg("activate descriptor is NULL");
    if (a->n < 0) return fail_msg("n < 0");
    if (a->reg) {
        if (int r = check_params_epsilon(a->epsilon)) return r;
        if (a->n == 0) return fail_msg("reg with n = 0: a mean over nothing");
    }
    if (a->n == 0) return 0;
    if (!a->scales && !a->rotations && !a->opacities && !a->reg)
        return fail_msg("no output requested (scales, rotations, opacities and reg are all NULL)");
    if ((a->scales && !a->scaling) || (a->rotations && !a->rotation) || ((a->opacities || a->reg) && !a->opacity))
        return fail_msg("NULL argument (scaling, rotation or opacity: the input of a requested output)");
    if (a->reg && !temp) return fail_msg("NULL argument (temp, needed with reg)");
    if (((uintptr_t)a->scaling | (uintptr_t)a->opacity | (uintptr_t)a->scales | (uintptr_t)a->opacities | (uintptr_t)a->reg) & 3)
        return fail_msg("scaling, opacity, scales, opacities and reg must be 4-byte aligned");
    if (((uintptr_t)a->rotation | (uintptr_t)a->rotations) & 15) return fail_msg("rotation and rotations must be 16-byte aligned");
    if (a->reg && ((uintptr_t)temp & 7)) return fail_msg("temp must be 8-byte aligned");
    if (a->reg && temp_bytes < params_temp_bytes(a->n)) return fail_msg("temp is smaller than texgs_params_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_activate", launch_params_activate(a, temp, s), s, false);
}

int texgs_params_activate_backward(const TexGSParamsActivateGrad* g, void* stream) {
    if (!g) return fail_msg("activate backward descriptor is NULL");
    if (g->n < 0) return fail_msg("n < 0");
    if (g->g_reg)
        if (int r = check_params_epsilon(g->epsilon)) return r;
    if (g->n == 0) return 0;
    if (!g->d_scaling && !g->d_rotation && !g->d_opacity)
        return fail_msg("no output requested (d_scaling, d_rotation and d_opacity are all NULL)");
    if ((g->d_scaling && g->g_scales && !g->scales) || (g->d_rotation && g->g_rotations && !g->rotation) ||
        (g->d_opacity && (g->g_opacities || g->g_reg) && !g->opacities))
        return fail_msg("NULL argument (scales, rotation or opacities: read for a requested output with an upstream gradient)");
    if (((uintptr_t)g->scales | (uintptr_t)g->opacities | (uintptr_t)g->g_scales | (uintptr_t)g->g_opacities | (uintptr_t)g->g_reg |
         (uintptr_t)g->d_scaling | (uintptr_t)g->d_opacity) & 3)
        return fail_msg("scales, opacities, g_scales, g_opacities, g_reg, d_scaling and d_opacity must be 4-byte aligned");
    if (((uintptr_t)g->rotation | (uintptr_t)g->g_rotations | (uintptr_t)g->d_rotation) & 15)
        return fail_msg("rotation, g_rotations and d_rotation must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_activate_backward", launch_params_activate_backward(g, s), s, false);
}

int texgs_params_covariance(const TexGSParamsCovariance* c, void* stream) {
    if (!c) return fail_msg("covariance descriptor is NULL");
    if (c->n < 0) return fail_msg("n < 0");
    if (int r = check_params_modifier(c->scale_modifier)) return r;
    if (c->n == 0) return 0;
    if (!c->scaling || !c->rotation || !c->cov) return fail_msg("NULL argument (scaling, rotation or cov)");
    if (((uintptr_t)c->scaling | (uintptr_t)c->cov) & 3) return fail_msg("scaling and cov must be 4-byte aligned");
    if ((uintptr_t)c->rotation & 15) return fail_msg("rotation must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_covariance", launch_params_covariance(c, s), s, false);
}

int texgs_params_covariance_backward(const TexGSParamsCovarianceGrad* c, void* stream) {
    if (!c) return fail_msg("covariance backward descriptor is NULL");
    if (c->n < 0) return fail_msg("n < 0");
    if (int r = check_params_modifier(c->scale_modifier)) return r;
    if (c->n == 0) return 0;
    if (!c->d_scaling && !c->d_rotation) return fail_msg("no output requested (d_scaling and d_rotation are both NULL)");
    if (!c->scaling || !c->rotation) return fail_msg("NULL argument (scaling or rotation)");
    if (((uintptr_t)c->scaling | (uintptr_t)c->g_cov | (uintptr_t)c->d_scaling) & 3) return fail_msg("scaling, g_cov and d_scaling must be 4-byte aligned");
    if (((uintptr_t)c->rotation | (uintptr_t)c->d_rotation) & 15) return fail_msg("rotation and d_rotation must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_covariance_backward", launch_params_covariance_backward(c, s), s, false);
}

}  // extern "C"
