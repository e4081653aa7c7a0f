// Exact spatial searches over an [N, 3] fp32 point cloud:
//   * mean squared distance to the three nearest other points -- what simple_knn's distCUDA2 returns and stage 1 initialises every
//     Gaussian's scale from (models/gaussian3d.py:63-64).  Algorithm restated from simple_knn's published description (Morton
//     order, boxes of consecutive points, box pruning), UNPINNED against the package;
//   * farthest-point sampling -- pytorch3d.ops.sample_farthest_points with random_start_point=False (extract_pcd.py:18-20),
//     restated, UNPINNED.
// The squared distance is part of a bit-exact contract: d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to fp32.  This unit
// is built with -ffp-contract=off so that no multiply-add pair is fused.
//
// Every dependency is a kernel boundary on the caller's stream: no spinning, no grid-wide barrier.  Every result is written by
// ordinary vector stores / vector atomics from device code.
#include "common.h"
#include "abi_support.h"
#include "wave_ops.h"

namespace {

constexpr int PT_BLOCK = 256;          // lanes per workgroup = points per box
constexpr int PT_BBOX_BLOCKS = 1024;   // workgroups of the bounding-box reduction (grid-stride)
// sub-slots per farthest-point pick: workgroup b posts its best to sub-slot b % FPS_SUB, the next step takes the largest.  Atomics on
// ONE address serialise (~13 ns each: 977 workgroups at N = 1 M); measured per pick at N = 300 k / 1 M: 1 -> 5.8 / 14.1 us,
// 16 -> 4.4 / 8.7 us, 64 -> 5.4 / 6.9 us (every lane reads all sub-slots of the previous pick)
constexpr int FPS_SUB = 16;
constexpr int FPS_PPL = 4;             // points per lane of one farthest-point step: 293 workgroups at N = 300 000 (1.14 per CU)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

__device__ __forceinline__ float pt_inf() { return __int_as_float(0x7f800000); }

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// keep the three smallest of {b0 <= b1 <= b2, d}, sorted
__device__ __forceinline__ void insert3(float& b0, float& b1, float& b2, float d) {
    const float t1 = fmaxf(b0, d);
    b0 = fminf(b0, d);
    const float t2 = fmaxf(b1, t1);
    b1 = fminf(b1, t1);
    b2 = fminf(b2, t2);
}

// order-preserving map of fp32 onto u32 (for integer atomic max)
__device__ __forceinline__ uint32_t f2ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) {
    return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// bbox (zeroed before the launch): words 0..2 = max of ~ord(x_c) (the minimum), words 3..5 = max of ord(x_c)
__global__ void __launch_bounds__(PT_BLOCK)
k_pt_bbox(const float* __restrict__ xyz, uint32_t n, uint32_t* __restrict__ bbox) {
    __shared__ float s_lo[4][3], s_hi[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float lo[3] = {pt_inf(), pt_inf(), pt_inf()}, hi[3] = {-pt_inf(), -pt_inf(), -pt_inf()};
    for (uint32_t i = blockIdx.x * PT_BLOCK + tid; i < n; i += gridDim.x * PT_BLOCK) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = xyz[(size_t)i * 3 + c];
            lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = wave_min_f(lo[c]); hi[c] = wave_max_f(hi[c]);
        if (lane == 0) { s_lo[wv][c] = lo[c]; s_hi[wv][c] = hi[c]; }
    }
    __syncthreads();
    if (tid < 3) {
        const float l = fminf(fminf(s_lo[0][tid], s_lo[1][tid]), fminf(s_lo[2][tid], s_lo[3][tid]));
        const float h = fmaxf(fmaxf(s_hi[0][tid], s_hi[1][tid]), fmaxf(s_hi[2][tid], s_hi[3][tid]));
        if (l <= h) {       // (a workgroup past the end of the cloud holds +inf / -inf)
            atomicMax(&bbox[tid], ~f2ord(l));
            atomicMax(&bbox[3 + tid], f2ord(h));
        }
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {      // bit k of a 10-bit value -> bit 3k
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit Morton code, 10 bits per axis over the bounding box; an axis of zero extent maps to cell 0.  The code only orders the
// search: the result does not depend on it.
__global__ void __launch_bounds__(PT_BLOCK)
k_pt_morton(const float* __restrict__ xyz, uint32_t n, const uint32_t* __restrict__ bbox, uint32_t* __restrict__ codes) {
    const uint32_t i = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t code = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = ord2f(~bbox[c]), hi = ord2f(bbox[3 + c]);
        const float ext = hi - lo;
        const float q = ext > 0.f ? (xyz[(size_t)i * 3 + c] - lo) / ext * 1023.f : 0.f;
        const uint32_t cell = (uint32_t)(int)fminf(fmaxf(q, 0.f), 1023.f);       // (fmaxf drops a NaN)
        code |= spread10(cell) << (2 - c);
    }
    codes[i] = code;
}

// One workgroup per box of 256 consecutive sorted points: gathers them into coordinate planes in sorted order and writes the box's
// componentwise min / max (bounds[b] = {lo xyz, hi xyz}).
__global__ void __launch_bounds__(PT_BLOCK)
k_pt_boxes(const float* __restrict__ xyz, const uint32_t* __restrict__ sidx, uint32_t n, float* __restrict__ sx, float* __restrict__ sy,
           float* __restrict__ sz, float* __restrict__ bounds) {
    __shared__ float s_lo[4][3], s_hi[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t i = blockIdx.x * PT_BLOCK + tid;
    const bool valid = i < n;
    float p[3] = {0.f, 0.f, 0.f};
    if (valid) {
        const uint32_t j = min(sidx[i], n - 1u);
        p[0] = xyz[(size_t)j * 3]; p[1] = xyz[(size_t)j * 3 + 1]; p[2] = xyz[(size_t)j * 3 + 2];
        sx[i] = p[0]; sy[i] = p[1]; sz[i] = p[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float l = wave_min_f(valid ? p[c] : pt_inf()), h = wave_max_f(valid ? p[c] : -pt_inf());
        if (lane == 0) { s_lo[wv][c] = l; s_hi[wv][c] = h; }
    }
    __syncthreads();
    if (tid < 3) {
        bounds[(size_t)blockIdx.x * 6 + tid] = fminf(fminf(s_lo[0][tid], s_lo[1][tid]), fminf(s_lo[2][tid], s_lo[3][tid]));
        bounds[(size_t)blockIdx.x * 6 + 3 + tid] = fmaxf(fmaxf(s_hi[0][tid], s_hi[1][tid]), fmaxf(s_hi[2][tid], s_hi[3][tid]));
    }
}

#ifdef TEXGS_POINTS_STATS
// Debug build only (-DTEXGS_POINTS_STATS; scripts/points_box_stats.py): how much of the cloud the search visits.
// [0] query boxes, [1] candidate boxes staged in LDS, summed over query boxes, [2] (lane, box) scans, [3] query points
__device__ unsigned long long g_pt_stats[4];
#endif

// One workgroup per query box, one query point per lane, its three smallest distances sorted in registers.
//   seed    the third smallest distance to the +-3 neighbours in sorted order is an upper bound (`reject`) of the lane's answer b2;
//   rounds  of 256 candidate boxes: lane l tests box (base + l) against the query box -- per-axis gap max(0, lo_c - hi_q, lo_q - hi_c)
//           in the d2 formula -- and the box is dropped for the whole workgroup when that bound is STRICTLY greater than the largest
//           threshold min(reject, b2) over the lanes;
//   a surviving box is staged in LDS (3 KiB, double-buffered: one barrier per box); a lane scans it unless the distance from its
//   point to the box (clamp to the box, same formula) is strictly greater than its own threshold.
// Neither bound can exceed the true d2 of any point of the box in fp32: each |component| is no larger than the point's and fp32
// subtract, multiply and add are monotone.  So a dropped box holds only points strictly farther than the lane's third neighbour.
__global__ void __launch_bounds__(PT_BLOCK)
k_pt_search(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const uint32_t* __restrict__ sidx,
            const float* __restrict__ bounds, uint32_t n, uint32_t nb, float* __restrict__ out) {
    __shared__ float s_p[2][3][PT_BLOCK];
    __shared__ float s_red[4];
    __shared__ unsigned long long s_mask[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t q = blockIdx.x;
    const uint32_t i = q * PT_BLOCK + tid;
    const bool valid = i < n;
    const float px = valid ? sx[i] : 0.f, py = valid ? sy[i] : 0.f, pz = valid ? sz[i] : 0.f;

    float reject = -1.f;                // a lane without a point passes no test (every bound is >= 0)
    if (valid) {
        float r0 = pt_inf(), r1 = pt_inf(), r2 = pt_inf();
#pragma unroll
        for (int o = -3; o <= 3; ++o) {
            if (o == 0) continue;
            const long long j = (long long)i + o;
            if (j >= 0 && j < (long long)n) insert3(r0, r1, r2, dist2(px, py, pz, sx[j], sy[j], sz[j]));
        }
        reject = r2;
    }
    float b0 = pt_inf(), b1 = pt_inf(), b2 = pt_inf();
    float qlo[3], qhi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { qlo[c] = bounds[(size_t)q * 6 + c]; qhi[c] = bounds[(size_t)q * 6 + 3 + c]; }

    uint32_t staged = 0u;               // boxes staged so far (workgroup-uniform): selects the LDS buffer
#ifdef TEXGS_POINTS_STATS
    uint32_t scans = 0u;
#endif
    for (uint32_t base = 0; base < nb; base += PT_BLOCK) {
        {
            const float wmax = wave_max_f(valid ? fminf(reject, b2) : -1.f);
            if (lane == 0) s_red[wv] = wmax;
        }
        __syncthreads();
        const float gmax = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        bool pass = false;
        const uint32_t cb = base + tid;
        if (cb < nb) {
            float g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float clo = bounds[(size_t)cb * 6 + c], chi = bounds[(size_t)cb * 6 + 3 + c];
                g[c] = fmaxf(0.f, fmaxf(clo - qhi[c], qlo[c] - chi));
            }
            const float bound = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
            pass = !(bound > gmax);
        }
        const unsigned long long mine = __ballot(pass);
        if (lane == 0) s_mask[wv] = mine;
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            const unsigned long long mw = s_mask[w];
            uint32_t mlo = __builtin_amdgcn_readfirstlane((uint32_t)mw), mhi = __builtin_amdgcn_readfirstlane((uint32_t)(mw >> 32));
            while (mlo | mhi) {
                int bit;
                if (mlo) { bit = __builtin_ctz(mlo); mlo &= mlo - 1u; }
                else { bit = 32 + __builtin_ctz(mhi); mhi &= mhi - 1u; }
                const uint32_t c = base + (uint32_t)w * 64u + (uint32_t)bit;        // < nb: only lanes with cb < nb set a bit
                const uint32_t first = c * PT_BLOCK;
                const uint32_t cnt = min((uint32_t)PT_BLOCK, n - first);
                const int buf = (int)(staged & 1u);
                ++staged;
                if ((uint32_t)tid < cnt) {
                    s_p[buf][0][tid] = sx[first + tid]; s_p[buf][1][tid] = sy[first + tid]; s_p[buf][2][tid] = sz[first + tid];
                }
                __syncthreads();
                const float thr = fminf(reject, b2);
                const float cx = fminf(fmaxf(px, bounds[(size_t)c * 6 + 0]), bounds[(size_t)c * 6 + 3]);
                const float cy = fminf(fmaxf(py, bounds[(size_t)c * 6 + 1]), bounds[(size_t)c * 6 + 4]);
                const float cz = fminf(fmaxf(pz, bounds[(size_t)c * 6 + 2]), bounds[(size_t)c * 6 + 5]);
                if (!(dist2(px, py, pz, cx, cy, cz) > thr)) {
#ifdef TEXGS_POINTS_STATS
                    ++scans;
#endif
                    const uint32_t self = i - first;            // >= cnt (or wrapped) unless this is the lane's own box
#pragma unroll 4
                    for (uint32_t j = 0; j < cnt; ++j) {
                        const float d = dist2(px, py, pz, s_p[buf][0][j], s_p[buf][1][j], s_p[buf][2][j]);
                        insert3(b0, b1, b2, j == self ? pt_inf() : d);
                    }
                }
            }
        }
    }
    if (valid) out[min(sidx[i], n - 1u)] = ((b0 + b1) + b2) / 3.0f;
#ifdef TEXGS_POINTS_STATS
    if (tid == 0) { atomicAdd(&g_pt_stats[0], 1ull); atomicAdd(&g_pt_stats[1], (unsigned long long)staged); }
    if (valid) { atomicAdd(&g_pt_stats[2], (unsigned long long)scans); atomicAdd(&g_pt_stats[3], 1ull); }
#endif
}

// Coordinate planes for the farthest-point steps: px / py / pz[j] = xyz[j][0 / 1 / 2] (the steps read four consecutive points per
// lane as 16-byte loads).
__global__ void __launch_bounds__(PT_BLOCK)
k_fps_planes(const float* __restrict__ xyz, uint32_t n, float* __restrict__ px, float* __restrict__ py, float* __restrict__ pz) {
    const uint32_t j = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (j >= n) return;
    px[j] = xyz[(size_t)j * 3]; py[j] = xyz[(size_t)j * 3 + 1]; pz[j] = xyz[(size_t)j * 3 + 2];
}

// One farthest-point step: m[j] = min(m[j], d2(xyz[j], xyz[previous pick])), then the workgroup's best (m, lowest j) goes to one of
// slot t's FPS_SUB sub-slots by a 64-bit atomic max of (bits of m << 32) | (0xFFFFFFFF - j): m >= 0, so its bits order like its
// value, and the largest key over the sub-slots is the pick (ties: the lowest j).  A lane owns FPS_PPL = 4
// consecutive points: four 16-byte loads and one 16-byte store.  The planes and m are padded to a multiple of 4 points; the padding
// is loaded and stored but never enters a key.
template <bool FIRST>
__global__ void __launch_bounds__(PT_BLOCK)
k_fps_step(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, uint32_t n, float* __restrict__ m,
           unsigned long long* __restrict__ slots, uint32_t t, uint32_t start) {
    static_assert(FPS_PPL == 4, "a lane reads its points as one float4 per plane");
    __shared__ unsigned long long s_best[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t j0 = (blockIdx.x * PT_BLOCK + tid) * FPS_PPL;
    const bool any = j0 < n;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x, z = x, mo = make_float4(pt_inf(), pt_inf(), pt_inf(), pt_inf());
    if (any) {                                   // all loads of the step in flight together, the previous pick's among them
        x = *reinterpret_cast<const float4*>(px + j0);
        y = *reinterpret_cast<const float4*>(py + j0);
        z = *reinterpret_cast<const float4*>(pz + j0);
        if (!FIRST) mo = *reinterpret_cast<const float4*>(m + j0);
    }
    uint32_t prev = start;
    if (!FIRST) {
        unsigned long long pk = 0ull;
#pragma unroll
        for (int u = 0; u < FPS_SUB; ++u) { const unsigned long long v = slots[(size_t)(t - 1) * FPS_SUB + u]; pk = v > pk ? v : pk; }
        prev = 0xFFFFFFFFu - (uint32_t)pk;
    }
    prev = min(prev, n - 1u);
    const float qx = px[prev], qy = py[prev], qz = pz[prev];
    unsigned long long best = 0ull;
    if (any) {
        const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w}, zs[4] = {z.x, z.y, z.z, z.w};
        float ms[4] = {mo.x, mo.y, mo.z, mo.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ms[u] = fminf(ms[u], dist2(xs[u], ys[u], zs[u], qx, qy, qz));
            const uint32_t j = j0 + (uint32_t)u;
            const unsigned long long key = ((unsigned long long)__float_as_uint(ms[u]) << 32) | (unsigned long long)(0xFFFFFFFFu - j);
            if (j < n && key > best) best = key;
        }
        *reinterpret_cast<float4*>(m + j0) = make_float4(ms[0], ms[1], ms[2], ms[3]);
    }
    best = wave_max_u64(best);
    if (lane == 0) s_best[wv] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = s_best[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) b = s_best[w] > b ? s_best[w] : b;
        unsigned long long* slot = &slots[(size_t)t * FPS_SUB + blockIdx.x % FPS_SUB];
        if (b != 0ull) atomicMax(slot, b);
    }
}

__global__ void __launch_bounds__(PT_BLOCK)
k_fps_unpack(const unsigned long long* __restrict__ slots, uint32_t k, uint32_t start, int32_t* __restrict__ idx) {
    const uint32_t t = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (t >= k) return;
    unsigned long long pk = 0ull;
#pragma unroll
    for (int u = 0; u < FPS_SUB; ++u) { const unsigned long long v = slots[(size_t)t * FPS_SUB + u]; pk = v > pk ? v : pk; }
    idx[t] = t == 0u ? (int32_t)start : (int32_t)(0xFFFFFFFFu - (uint32_t)pk);
}

struct KnnTemp {
    uint32_t *bbox, *codes, *skeys, *sidx;
    float *sx, *sy, *sz, *bounds;
    void* sort;
    size_t bytes;
};

KnnTemp knn_temp(void* base, uint32_t n) {
    KnnTemp t;
    char* p = (char*)base;
    const size_t nb4 = align256((size_t)n * 4);
    t.bbox = (uint32_t*)p; p += 256;
    t.codes = (uint32_t*)p; p += nb4;
    t.skeys = (uint32_t*)p; p += nb4;
    t.sidx = (uint32_t*)p; p += nb4;
    t.sx = (float*)p; p += nb4;
    t.sy = (float*)p; p += nb4;
    t.sz = (float*)p; p += nb4;
    t.bounds = (float*)p; p += align256((size_t)((n + PT_BLOCK - 1) / PT_BLOCK) * 6 * 4);
    t.sort = p; p += sort_pairs32_temp_bytes(n);
    t.bytes = (size_t)(p - (char*)base);
    return t;
}

}  // namespace

static size_t knn3_temp_bytes(int n) { return knn_temp(nullptr, (uint32_t)(n > 0 ? n : 1)).bytes; }

static hipError_t launch_knn3_mean_dist2(const float* xyz, int n_, float* mean_d2, void* temp, hipStream_t s) {
    const uint32_t n = (uint32_t)n_;
    const KnnTemp t = knn_temp(temp, n);
    const uint32_t nb = (n + PT_BLOCK - 1) / PT_BLOCK;
    if (hipError_t e = hipMemsetAsync(t.bbox, 0, 256, s)) return e;
    hipLaunchKernelGGL(k_pt_bbox, dim3(nb < (uint32_t)PT_BBOX_BLOCKS ? nb : (uint32_t)PT_BBOX_BLOCKS), dim3(PT_BLOCK), 0, s, xyz, n, t.bbox);
    hipLaunchKernelGGL(k_pt_morton, dim3(nb), dim3(PT_BLOCK), 0, s, xyz, n, (const uint32_t*)t.bbox, t.codes);
    if (hipError_t e = launch_sort_pairs32(t.codes, n, 30, t.skeys, t.sidx, t.sort, s)) return e;
    hipLaunchKernelGGL(k_pt_boxes, dim3(nb), dim3(PT_BLOCK), 0, s, xyz, (const uint32_t*)t.sidx, n, t.sx, t.sy, t.sz, t.bounds);
    hipLaunchKernelGGL(k_pt_search, dim3(nb), dim3(PT_BLOCK), 0, s, (const float*)t.sx, (const float*)t.sy, (const float*)t.sz,
                       (const uint32_t*)t.sidx, (const float*)t.bounds, n, nb, mean_d2);
    return hipGetLastError();
}

// temp: m, px, py, pz (n floats each, padded to 256 bytes: a multiple of 4 points), then k x FPS_SUB 64-bit slots
static size_t fps_temp_bytes(int n, int k) {
    return 4 * align256((size_t)(n > 0 ? n : 1) * 4) + align256((size_t)(k > 0 ? k : 1) * 8 * FPS_SUB);
}

static hipError_t launch_farthest_points(const float* xyz, int n_, int k_, int start, int32_t* idx, void* temp, hipStream_t s) {
    const uint32_t n = (uint32_t)n_, k = (uint32_t)k_;
    const size_t plane = align256((size_t)n * 4);
    float* m = (float*)temp;
    float* px = (float*)((char*)temp + plane);
    float* py = (float*)((char*)temp + 2 * plane);
    float* pz = (float*)((char*)temp + 3 * plane);
    unsigned long long* slots = (unsigned long long*)((char*)temp + 4 * plane);
    if (hipError_t e = hipMemsetAsync(slots, 0, (size_t)k * 8 * FPS_SUB, s)) return e;
    if (k > 1) hipLaunchKernelGGL(k_fps_planes, dim3((n + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, s, xyz, n, px, py, pz);
    const uint32_t grid = (n + PT_BLOCK * FPS_PPL - 1) / (PT_BLOCK * FPS_PPL);
    for (uint32_t t = 1; t < k; ++t) {
        if (t == 1)
            hipLaunchKernelGGL(k_fps_step<true>, dim3(grid), dim3(PT_BLOCK), 0, s, (const float*)px, (const float*)py, (const float*)pz, n, m,
                               slots, t, (uint32_t)start);
        else
            hipLaunchKernelGGL(k_fps_step<false>, dim3(grid), dim3(PT_BLOCK), 0, s, (const float*)px, (const float*)py, (const float*)pz, n, m,
                               slots, t, (uint32_t)start);
    }
    hipLaunchKernelGGL(k_fps_unpack, dim3((k + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, s, (const unsigned long long*)slots, k,
                       (uint32_t)start, idx);
    return hipGetLastError();
}

extern "C" {

size_t texgs_knn3_temp_bytes(int32_t n) { return knn3_temp_bytes(n); }

int texgs_knn3_mean_dist2(const float* xyz, int32_t n, float* mean_d2, void* temp, void* stream) {
    if (n < 4) return fail_msg("n < 4: three nearest other points need at least four points");
    if (!xyz || !mean_d2 || !temp) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("knn3_mean_dist2", launch_knn3_mean_dist2(xyz, n, mean_d2, temp, s), s, false);
}

size_t texgs_fps_temp_bytes(int32_t n, int32_t k) { return fps_temp_bytes(n, k); }

int texgs_farthest_points(const float* xyz, int32_t n, int32_t k, int32_t start, int32_t* idx, void* temp, void* stream) {
    if (n < 1) return fail_msg("n < 1");
    if (k < 1 || k > n) return fail_msg("k must be in [1, n]");
    if (start < 0 || start >= n) return fail_msg("start must be in [0, n)");
    if (!xyz || !idx || !temp) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("farthest_points", launch_farthest_points(xyz, n, k, start, idx, temp, s), s, false);
}

}  // extern "C"

#ifdef TEXGS_POINTS_STATS
// Debug build only: read (and optionally zero) the search counters; synchronises the device.
extern "C" int texgs_points_stats(unsigned long long* out4, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out4 && hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_pt_stats), 32) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_pt_stats), z, 32) != hipSuccess) return -1;
    }
    return 0;
}
#endif
