// UV-map stage (stage 2 of Texture-GS, models/uv_map_gaussian3d.py:167-238): the multiresolution hash-grid encoding of InvUVNet
// (models/modules/utils.py:5-29, tiny-cuda-nn "HashGrid", F = 4 features per level) forward and backward, and the nearest-neighbour
// search of the chamfer loss (pytorch3d.loss.chamfer_distance, batch 1, squared L2).  The grid's index rules are restated from
// tiny-cuda-nn's published grid encoding (UNPINNED against the package).
//
// Every result is written by ordinary vector stores / vector atomics from device code; nothing here uses the scalar memory path.
#include "common.h"
#include "abi_support.h"

#include <algorithm>

static int hashgrid_levels(const TexGSHashGrid* g, float* scale, uint32_t* res, uint32_t* size, uint32_t* offset, uint32_t* n_params);

namespace {

// a level whose gradient slab (size_l rows x 16 B) fits is accumulated in LDS: 64 KiB, two workgroups per CU
constexpr uint64_t HG_LDS_MAX_BYTES = 65536;

constexpr int HG_FWD_BLOCK = 256;
constexpr int HG_BWD_BLOCK = 512;
constexpr int NN_BLOCK = 256;
constexpr int NN_SPLIT = 512;          // reference points per workgroup (LDS: 6 KiB)

struct HGDev {                          // per-level constants, passed by value
    int L;
    float scale[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t res[TEXGS_HASHGRID_MAX_LEVELS], size[TEXGS_HASHGRID_MAX_LEVELS], offset[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t hashed[TEXGS_HASHGRID_MAX_LEVELS];
};

struct HGSel {                          // levels one backward launch covers (blockIdx.y -> level)
    int n;
    int level[TEXGS_HASHGRID_MAX_LEVELS];
};

__device__ __forceinline__ uint32_t hg_index(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t res, uint32_t size, uint32_t hashed) {
    const uint32_t i = hashed ? (p0 ^ (p1 * 2654435761u) ^ (p2 * 805459861u)) : (p0 + p1 * res + p2 * (res * res));
    return i % size;
}

// cell corner and fractions of point i at level l (no clamping: any corner is wrapped into the level by % size)
__device__ __forceinline__ void hg_cell(const HGDev& g, int l, const float* __restrict__ x, uint32_t i, uint32_t p[3], float f[3]) {
    const float s = g.scale[l];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float pos = fmaf(s, x[(size_t)i * 3 + d], 0.5f);
        const float fl = floorf(pos);
        p[d] = (uint32_t)(int)fl;
        f[d] = pos - fl;
    }
}

__global__ void __launch_bounds__(HG_FWD_BLOCK)
k_hg_forward(HGDev g, const float* __restrict__ params, const float* __restrict__ x, uint32_t N, float* __restrict__ enc) {
    const uint32_t t = blockIdx.x * HG_FWD_BLOCK + threadIdx.x;       // (point, level), level fastest
    if (t >= N * (uint32_t)g.L) return;
    const uint32_t i = t / g.L;
    const int l = t - i * g.L;
    uint32_t p[3];
    float f[3];
    hg_cell(g, l, x, i, p, f);
    const uint32_t res = g.res[l], size = g.size[l], hashed = g.hashed[l];
    const float4* tab = reinterpret_cast<const float4*>(params) + g.offset[l];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int c0 = c & 1, c1 = (c >> 1) & 1, c2 = c >> 2;
        const float w = (c0 ? f[0] : 1.f - f[0]) * (c1 ? f[1] : 1.f - f[1]) * (c2 ? f[2] : 1.f - f[2]);
        const float4 th = tab[hg_index(p[0] + c0, p[1] + c1, p[2] + c2, res, size, hashed)];
        acc.x = fmaf(w, th.x, acc.x); acc.y = fmaf(w, th.y, acc.y); acc.z = fmaf(w, th.z, acc.z); acc.w = fmaf(w, th.w, acc.w);
    }
    reinterpret_cast<float4*>(enc)[(size_t)i * g.L + l] = acc;         // 8 lanes of a point: 128 contiguous bytes (L = 8)
}

// One workgroup = (one level, one chunk of points).  LDS = true: the level's gradient slab (size_l rows x 4 floats) is accumulated
// with LDS float atomics and flushed once with contiguous global float atomics; LDS = false: one global float atomic per corner and
// feature (levels whose slab does not fit).  dxl: the level's share of d enc / d x, [L][N][3], plain stores.
template <bool LDS>
__global__ void __launch_bounds__(HG_BWD_BLOCK)
k_hg_backward(HGDev g, HGSel sel, const float* __restrict__ params, const float* __restrict__ x, const float* __restrict__ d_enc,
              uint32_t N, uint32_t per_chunk, float* __restrict__ d_params, float* __restrict__ dxl) {
    extern __shared__ float slab[];
    const int l = sel.level[blockIdx.y];
    const uint32_t res = g.res[l], size = g.size[l], hashed = g.hashed[l];
    const float4* tab = reinterpret_cast<const float4*>(params) + g.offset[l];
    float* dtab = d_params ? d_params + (size_t)g.offset[l] * 4 : nullptr;
    if (LDS && dtab) {
        for (uint32_t k = threadIdx.x; k < size * 4; k += HG_BWD_BLOCK) slab[k] = 0.f;
        __syncthreads();
    }
    const uint32_t begin = blockIdx.x * per_chunk;
    const uint32_t end = min(N, begin + per_chunk);
    for (uint32_t i = begin + threadIdx.x; i < end; i += HG_BWD_BLOCK) {
        uint32_t p[3];
        float f[3];
        hg_cell(g, l, x, i, p, f);
        const float4 de = reinterpret_cast<const float4*>(d_enc)[(size_t)i * g.L + l];
        float dx0 = 0.f, dx1 = 0.f, dx2 = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int c0 = c & 1, c1 = (c >> 1) & 1, c2 = c >> 2;
            const float w0 = c0 ? f[0] : 1.f - f[0], w1 = c1 ? f[1] : 1.f - f[1], w2 = c2 ? f[2] : 1.f - f[2];
            const uint32_t idx = hg_index(p[0] + c0, p[1] + c1, p[2] + c2, res, size, hashed);
            if (dtab) {
                const float w = w0 * w1 * w2;
                if (LDS) {
                    atomicAdd(&slab[idx * 4 + 0], w * de.x); atomicAdd(&slab[idx * 4 + 1], w * de.y);
                    atomicAdd(&slab[idx * 4 + 2], w * de.z); atomicAdd(&slab[idx * 4 + 3], w * de.w);
                } else {
                    float* r = dtab + (size_t)idx * 4;
                    atomicAdd(r + 0, w * de.x); atomicAdd(r + 1, w * de.y); atomicAdd(r + 2, w * de.z); atomicAdd(r + 3, w * de.w);
                }
            }
            if (dxl) {
                const float4 th = tab[idx];
                const float s = th.x * de.x + th.y * de.y + th.z * de.z + th.w * de.w;
                dx0 += (c0 ? s : -s) * (w1 * w2);
                dx1 += (c1 ? s : -s) * (w0 * w2);
                dx2 += (c2 ? s : -s) * (w0 * w1);
            }
        }
        if (dxl) {
            const float sc = g.scale[l];
            float* o = dxl + ((size_t)l * N + i) * 3;
            o[0] = sc * dx0; o[1] = sc * dx1; o[2] = sc * dx2;
        }
    }
    if (LDS && dtab) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < size * 4; k += HG_BWD_BLOCK) {
            const float v = slab[k];
            if (v != 0.f) atomicAdd(dtab + k, v);
        }
    }
}

__global__ void __launch_bounds__(256)
k_hg_dx_reduce(const float* __restrict__ dxl, int L, uint32_t N, float* __restrict__ dx) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;                // element of [N, 3]
    if (t >= N * 3) return;
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += dxl[(size_t)l * N * 3 + t];      // fixed level order: deterministic
    dx[t] = s;
}

// Nearest neighbour of each a_i in b[j0, j0 + NN_SPLIT): d = sum_d (a_d - b_d)^2, the lowest j on ties inside the split, then a
// 64-bit atomic min on (d bits << 32 | j) across splits (d >= 0, so its bits order like the value; ties -> lowest j).
__global__ void __launch_bounds__(NN_BLOCK)
k_nn_search(const float* __restrict__ a, uint32_t P, const float* __restrict__ b, uint32_t Q, unsigned long long* __restrict__ keys) {
    __shared__ float sb[NN_SPLIT * 3];
    const uint32_t j0 = blockIdx.y * NN_SPLIT;
    const uint32_t nj = min((uint32_t)NN_SPLIT, Q - j0);
    for (uint32_t k = threadIdx.x; k < nj * 3; k += NN_BLOCK) sb[k] = b[(size_t)j0 * 3 + k];
    __syncthreads();
    const uint32_t i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= P) return;
    const float ax = a[(size_t)i * 3], ay = a[(size_t)i * 3 + 1], az = a[(size_t)i * 3 + 2];
    float best = __int_as_float(0x7f800000);
    int bj = -1;
    for (uint32_t j = 0; j < nj; ++j) {
        const float dx = ax - sb[j * 3], dy = ay - sb[j * 3 + 1], dz = az - sb[j * 3 + 2];
        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        if (d < best) { best = d; bj = (int)j; }
    }
    if (bj >= 0) atomicMin(&keys[i], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(j0 + bj));
}

__global__ void __launch_bounds__(256)
k_nn_unpack(const unsigned long long* __restrict__ keys, uint32_t P, float* __restrict__ d2, int32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const unsigned long long k = keys[i];
    const bool none = k == ~0ull;          // no finite distance (non-finite input): NaN distance, a valid index
    d2[i] = none ? __int_as_float(0x7fc00000) : __uint_as_float((uint32_t)(k >> 32));
    idx[i] = none ? 0 : (int32_t)(uint32_t)k;
}

int hg_device_table(const TexGSHashGrid* g, HGDev* d) {
    uint32_t total = 0;
    float scale[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t res[TEXGS_HASHGRID_MAX_LEVELS], size[TEXGS_HASHGRID_MAX_LEVELS], off[TEXGS_HASHGRID_MAX_LEVELS];
    if (int r = hashgrid_levels(g, scale, res, size, off, &total)) return r;
    d->L = g->n_levels;
    for (int l = 0; l < d->L; ++l) {
        d->scale[l] = scale[l]; d->res[l] = res[l]; d->size[l] = size[l]; d->offset[l] = off[l];
        d->hashed[l] = (uint64_t)res[l] * res[l] * res[l] > size[l];
    }
    return 0;
}

int cu_count() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    return n;
}

}  // namespace

static int hashgrid_levels(const TexGSHashGrid* g, float* scale, uint32_t* res, uint32_t* size, uint32_t* offset, uint32_t* n_params) {
    if (g->n_levels < 1 || g->n_levels > TEXGS_HASHGRID_MAX_LEVELS) return -1;
    if (g->n_features != TEXGS_HASHGRID_FEATURES) return -2;
    if (g->log2_hashmap_size < 1 || g->log2_hashmap_size > 24) return -3;
    if (!(g->base_resolution >= 1.f) || !(g->per_level_scale >= 1.f) || !(g->per_level_scale <= 16.f)) return -4;
    const float lpls = log2f(g->per_level_scale);
    const uint64_t T = 1ull << g->log2_hashmap_size;
    uint64_t total = 0;
    for (int l = 0; l < g->n_levels; ++l) {
        const float s = exp2f((float)l * lpls) * g->base_resolution - 1.0f;
        if (!(s >= 0.f) || !(s < 2097150.f)) return -5;             // res^3 fits in 64 bits; % size runs in 32
        const uint64_t r = (uint64_t)ceilf(s) + 1;
        const uint64_t dense = r * r * r;
        const uint64_t sz = std::min<uint64_t>((dense + 7) & ~7ull, T);
        scale[l] = s; res[l] = (uint32_t)r; size[l] = (uint32_t)sz; offset[l] = (uint32_t)total;
        total += sz;
        if (total * 4 > 0x7fffffffull) return -6;
    }
    *n_params = (uint32_t)(total * 4);
    return 0;
}

static hipError_t launch_hashgrid_forward(const TexGSHashGrid* g, const float* params, const float* x, int N, float* enc, hipStream_t s) {
    HGDev d;
    if (hg_device_table(g, &d)) return hipErrorInvalidValue;      // (check_hashgrid below rejects such a grid first, with the reason)
    const uint64_t lanes = (uint64_t)N * d.L;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hg_forward, dim3((uint32_t)((lanes + HG_FWD_BLOCK - 1) / HG_FWD_BLOCK)), dim3(HG_FWD_BLOCK), 0, s, d, params, x,
                       (uint32_t)N, enc);
    return hipGetLastError();
}

static size_t hashgrid_backward_temp_bytes(const TexGSHashGrid* g, int N) {
    return (size_t)g->n_levels * (size_t)(N > 0 ? N : 0) * 3 * sizeof(float);
}

static hipError_t launch_hashgrid_backward(const TexGSHashGrid* g, const float* params, const float* x, const float* d_enc, int N, float* d_params,
                             float* d_x, void* temp, hipStream_t s) {
    HGDev d;
    if (hg_device_table(g, &d)) return hipErrorInvalidValue;
    if (N == 0 || (!d_params && !d_x)) return hipSuccess;
    float* dxl = d_x ? (float*)temp : nullptr;
    HGSel lds = {}, glob = {};
    uint32_t lds_max = 0;
    for (int l = 0; l < d.L; ++l) {
        const bool fits = d_params && (uint64_t)d.size[l] * 16 <= HG_LDS_MAX_BYTES;
        HGSel& t = fits ? lds : glob;
        t.level[t.n++] = l;
        if (fits) lds_max = std::max(lds_max, d.size[l] * 16);
    }
    // two workgroups of 512 lanes per CU (64 KiB slabs: 2 x 64 of 160 KiB): one wave of workgroups over the chip
    const uint32_t cus = (uint32_t)cu_count();
    auto launch = [&](const HGSel& t, bool use_lds) {
        if (t.n == 0) return;
        uint32_t chunks = std::max(1u, (2 * cus + t.n - 1) / t.n);
        chunks = std::min(chunks, ((uint32_t)N + HG_BWD_BLOCK - 1) / HG_BWD_BLOCK);
        const uint32_t per = ((uint32_t)N + chunks - 1) / chunks;
        chunks = ((uint32_t)N + per - 1) / per;
        if (use_lds)
            hipLaunchKernelGGL(k_hg_backward<true>, dim3(chunks, t.n), dim3(HG_BWD_BLOCK), lds_max, s, d, t, params, x, d_enc,
                               (uint32_t)N, per, d_params, dxl);
        else
            hipLaunchKernelGGL(k_hg_backward<false>, dim3(chunks, t.n), dim3(HG_BWD_BLOCK), 0, s, d, t, params, x, d_enc,
                               (uint32_t)N, per, d_params, dxl);
    };
    launch(lds, true);
    launch(glob, false);
    if (d_x)
        hipLaunchKernelGGL(k_hg_dx_reduce, dim3(((uint32_t)N * 3 + 255) / 256), dim3(256), 0, s, (const float*)dxl, d.L, (uint32_t)N, d_x);
    return hipGetLastError();
}

static size_t chamfer_nn_temp_bytes(int P) { return (size_t)(P > 0 ? P : 0) * sizeof(unsigned long long); }

static hipError_t launch_chamfer_nn(const float* a, int P, const float* b, int Q, float* d2, int32_t* idx, void* temp, hipStream_t s) {
    if (P == 0) return hipSuccess;
    unsigned long long* keys = (unsigned long long*)temp;
    if (hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)P * sizeof(unsigned long long), s)) return e;
    hipLaunchKernelGGL(k_nn_search, dim3(((uint32_t)P + NN_BLOCK - 1) / NN_BLOCK, ((uint32_t)Q + NN_SPLIT - 1) / NN_SPLIT), dim3(NN_BLOCK),
                       0, s, a, (uint32_t)P, b, (uint32_t)Q, keys);
    hipLaunchKernelGGL(k_nn_unpack, dim3(((uint32_t)P + 255) / 256), dim3(256), 0, s, (const unsigned long long*)keys, (uint32_t)P, d2, idx);
    return hipGetLastError();
}

extern "C" {

static int check_hashgrid(const TexGSHashGrid* g, uint32_t* n_params) {
    if (!g) return fail_msg("grid is NULL");
    float sc[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t r[TEXGS_HASHGRID_MAX_LEVELS], sz[TEXGS_HASHGRID_MAX_LEVELS], off[TEXGS_HASHGRID_MAX_LEVELS];
    switch (hashgrid_levels(g, sc, r, sz, off, n_params)) {
    case 0: return 0;
    case -1: return fail_msg("hash grid: n_levels must be in [1, 16]");
    case -2: return fail_msg("hash grid: n_features must be 4");
    case -3: return fail_msg("hash grid: log2_hashmap_size must be in [1, 24]");
    case -4: return fail_msg("hash grid: base_resolution must be >= 1 and per_level_scale in [1, 16]");
    case -5: return fail_msg("hash grid: a level's resolution is out of range");
    default: return fail_msg("hash grid: more than 2^31 parameters");
    }
}

int texgs_hashgrid_levels(const TexGSHashGrid* grid, float* scale, uint32_t* res, uint32_t* size, uint32_t* offset, uint32_t* n_params) {
    uint32_t n = 0;
    if (int r = check_hashgrid(grid, &n)) return r;
    float sc[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t rs[TEXGS_HASHGRID_MAX_LEVELS], sz[TEXGS_HASHGRID_MAX_LEVELS], off[TEXGS_HASHGRID_MAX_LEVELS];
    hashgrid_levels(grid, sc, rs, sz, off, &n);
    for (int l = 0; l < grid->n_levels; ++l) {
        if (scale) scale[l] = sc[l];
        if (res) res[l] = rs[l];
        if (size) size[l] = sz[l];
        if (offset) offset[l] = off[l];
    }
    if (n_params) *n_params = n;
    return 0;
}

int texgs_hashgrid_forward(const TexGSHashGrid* grid, const float* params, const float* x, int32_t N, float* enc, void* stream) {
    uint32_t n = 0;
    if (int r = check_hashgrid(grid, &n)) return r;
    if (N < 0) return fail_msg("N < 0");
    if ((int64_t)N * grid->n_levels * TEXGS_HASHGRID_FEATURES > INT32_MAX) return fail_msg("N * L * F >= 2^31");
    if (N > 0 && (!params || !x || !enc)) return fail_msg("NULL argument");
    if (N > 0 && (((uintptr_t)params | (uintptr_t)enc) & 15)) return fail_msg("params and enc must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("hashgrid_forward", launch_hashgrid_forward(grid, params, x, N, enc, s), s, false);
}

size_t texgs_hashgrid_backward_temp_bytes(const TexGSHashGrid* grid, int32_t N) {
    uint32_t n = 0;
    if (!grid || check_hashgrid(grid, &n)) return 0;
    return hashgrid_backward_temp_bytes(grid, N);
}

int texgs_hashgrid_backward(const TexGSHashGrid* grid, const float* params, const float* x, const float* d_enc, int32_t N,
                            float* d_params, float* d_x, void* temp, void* stream) {
    uint32_t n = 0;
    if (int r = check_hashgrid(grid, &n)) return r;
    if (N < 0) return fail_msg("N < 0");
    if ((int64_t)N * grid->n_levels * TEXGS_HASHGRID_FEATURES > INT32_MAX) return fail_msg("N * L * F >= 2^31");
    if (N > 0 && (!params || !x || !d_enc)) return fail_msg("NULL argument");
    if (N > 0 && (((uintptr_t)params | (uintptr_t)d_enc | (uintptr_t)d_params) & 15))
        return fail_msg("params, d_enc and d_params must be 16-byte aligned");
    if (N > 0 && d_x && !temp) return fail_msg("temp is NULL (d_x needs texgs_hashgrid_backward_temp_bytes)");
    hipStream_t s = (hipStream_t)stream;
    return launched("hashgrid_backward", launch_hashgrid_backward(grid, params, x, d_enc, N, d_params, d_x, temp, s), s, false);
}

size_t texgs_chamfer_nn_temp_bytes(int32_t P) { return chamfer_nn_temp_bytes(P); }

int texgs_chamfer_nn(const float* a, int32_t P, const float* b, int32_t Q, float* d2, int32_t* idx, void* temp, void* stream) {
    if (P < 0) return fail_msg("P < 0");
    if (Q < 1) return fail_msg("the reference set is empty (Q < 1)");
    if ((int64_t)Q > 65535ll * 512) return fail_msg("Q > 65535 * 512");
    if (P > 0 && (!a || !b || !d2 || !idx || !temp)) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("chamfer_nn", launch_chamfer_nn(a, P, b, Q, d2, idx, temp, s), s, false);
}

}  // extern "C"
