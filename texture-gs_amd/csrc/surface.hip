// The surface-point stage (include/texgs_surface.h): depth map -> world points of the pixels whose alpha passes a threshold, in pixel
// order (models/uv_map_gaussian3d.py:180-183, :271-286 of the reference), and the composite that puts per-point colours back onto the
// pixel grid.  Built with -ffp-contract=off: the fp64 inverse, the fp64 dot products and the fp32 composite are compared bit for bit
// with tests/surface_ref.py ('/' is the correctly rounded division here, for double as for float).
//
// The compaction is csrc/density.hip's three plain launches: no global atomics and no workgroup waits on another.
//   1. k_surface_count   a workgroup counts the selected pixels among its SF_TILE pixels: 64-bit ballots, popcount
//   2. k_surface_scan    ONE workgroup turns the counts into exclusive offsets (SF_SCAN per pass, running carry), writes the total
//                        and the twelve fp64 entries of the inverse projection into temp
//   3. k_surface_write   re-forms the ballots, ranks the lanes (mbcnt) and writes xyz / index / alpha / rank
// A thread takes 4 consecutive pixels, so its selected pixels have consecutive ranks and a workgroup's rows are one contiguous run:
// the 12-byte xyz rows are staged in LDS and stored as dense dwords.
#include "common.h"
#include "abi_support.h"
#include "texgs_surface.h"

namespace {

constexpr int SF_BLOCK = 256;
constexpr int SF_ITEMS = TEXGS_SURFACE_PIXELS_PER_THREAD;
constexpr int SF_TILE = TEXGS_SURFACE_PIXELS_PER_WORKGROUP;
constexpr int SF_SCAN = TEXGS_SURFACE_SCAN_WIDTH;
constexpr int SF_WAVES = SF_BLOCK / 64;
constexpr size_t SF_INV_BYTES = 12 * sizeof(double);        // temp: the inverse's columns 0..2, then one uint32 per workgroup
static_assert(SF_TILE == SF_BLOCK * SF_ITEMS && SF_ITEMS == 4 && SF_SCAN == SF_BLOCK, "the constants of texgs_surface.h");

// 4 consecutive elements from p0 (a multiple of 4): one 16-byte load where the plane allows it; elements at and past n read as `pad`
template <typename T, typename V4>
__device__ __forceinline__ void load4(const T* __restrict__ base, uint32_t p0, uint32_t n, bool vec, T pad, T v[4]) {
    if (vec && p0 + 3 < n) {
        const V4 q = *reinterpret_cast<const V4*>(base + p0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p0 + k < n ? base[p0 + k] : pad;
    }
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the thread's four selection bits and, per item, the wave's ballot
__device__ __forceinline__ void select4(const float* __restrict__ alpha, uint32_t p0, uint32_t n, bool vec, float thr, float a[4],
                                        bool sel[4], unsigned long long bal[4]) {
    load4<float, float4>(alpha, p0, n, vec, 0.0f, a);
#pragma unroll
    for (int k = 0; k < SF_ITEMS; ++k) {
        sel[k] = (p0 + k < n) && (a[k] > thr);          // strict: a NaN alpha is not selected
        bal[k] = __ballot(sel[k]);
    }
}

// launch 1
__global__ void __launch_bounds__(SF_BLOCK)
k_surface_count(const float* __restrict__ alpha, uint32_t n, int vec, float thr, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_wave[SF_WAVES];
    const uint32_t p0 = blockIdx.x * SF_TILE + threadIdx.x * SF_ITEMS;
    float a[4]; bool sel[4]; unsigned long long bal[4];
    select4(alpha, p0, n, vec != 0, thr, a, sel, bal);
    if ((threadIdx.x & 63) == 0)
        s_wave[threadIdx.x >> 6] = (uint32_t)(__popcll(bal[0]) + __popcll(bal[1]) + __popcll(bal[2]) + __popcll(bal[3]));
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < SF_WAVES; ++w) c += s_wave[w];
        counts[blockIdx.x] = c;
    }
}

__device__ __forceinline__ double term3(double p, double q, double r, double u, double v, double w) { return ((p * u) - (q * v)) + (r * w); }

// launch 2: one workgroup.  counts[t] becomes the number of selected pixels in the workgroups before t.
__global__ void __launch_bounds__(SF_SCAN)
k_surface_scan(uint32_t* __restrict__ counts, uint32_t tiles, uint32_t* __restrict__ total, const float* __restrict__ full_proj,
               double* __restrict__ inv) {
    __shared__ uint32_t s_wave[SF_SCAN / 64];
    if (threadIdx.x == SF_SCAN - 1) {        // the inverse's columns 0..2 (texgs_surface.h states the order): inv[3 i + j] = B_ij
        double a[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) a[k] = (double)full_proj[k];
        const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
        const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
        const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
        const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
        const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
        inv[0] = term3(a[5], a[6], a[7], c5, c4, c3) / det;
        inv[1] = -term3(a[1], a[2], a[3], c5, c4, c3) / det;
        inv[2] = term3(a[13], a[14], a[15], s5, s4, s3) / det;
        inv[3] = -term3(a[4], a[6], a[7], c5, c2, c1) / det;
        inv[4] = term3(a[0], a[2], a[3], c5, c2, c1) / det;
        inv[5] = -term3(a[12], a[14], a[15], s5, s2, s1) / det;
        inv[6] = term3(a[4], a[5], a[7], c4, c2, c0) / det;
        inv[7] = -term3(a[0], a[1], a[3], c4, c2, c0) / det;
        inv[8] = term3(a[12], a[13], a[15], s4, s2, s0) / det;
        inv[9] = -term3(a[4], a[5], a[6], c3, c1, c0) / det;
        inv[10] = term3(a[0], a[1], a[2], c3, c1, c0) / det;
        inv[11] = -term3(a[12], a[13], a[14], s3, s1, s0) / det;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < tiles; first += SF_SCAN) {
        const uint32_t t = first + threadIdx.x;
        const uint32_t v = t < tiles ? counts[t] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SF_SCAN / 64; ++w) {
            const uint32_t s = s_wave[w];
            if (w < wave) before += s;
            all += s;
        }
        if (t < tiles) counts[t] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

struct WriteArgs {
    const float* depth; const float* alpha; const double* inv; const uint32_t* offsets;
    float* xyz; int64_t* index; float* alpha_sel; int32_t* rank;
    uint32_t n, width;
    int vec_alpha, vec_depth;
    float thr;
    double zfar, zk, zb, fw, fh;        // zk = zfar - znear, zb = (zfar znear) / zk: both rounded once, on the host
};

// launch 3
__global__ void __launch_bounds__(SF_BLOCK)
k_surface_write(WriteArgs g) {
    __shared__ uint32_t s_wave[SF_WAVES];
    __shared__ float s_xyz[3 * SF_TILE];
    const uint32_t p0 = blockIdx.x * SF_TILE + threadIdx.x * SF_ITEMS;
    const int wave = threadIdx.x >> 6;
    float a[4]; bool sel[4]; unsigned long long bal[4];
    select4(g.alpha, p0, g.n, g.vec_alpha != 0, g.thr, a, sel, bal);
    uint32_t below = 0, in_wave = 0;
#pragma unroll
    for (int k = 0; k < SF_ITEMS; ++k) {
        below += lanes_below(bal[k]);
        in_wave += (uint32_t)__popcll(bal[k]);
    }
    if ((threadIdx.x & 63) == 0) s_wave[wave] = in_wave;
    __syncthreads();
    const uint32_t rb = g.offsets[blockIdx.x];          // the workgroup's first row; cb: its number of rows
    uint32_t r = rb + below, cb = 0;
#pragma unroll
    for (int w = 0; w < SF_WAVES; ++w) {
        if (w < wave) r += s_wave[w];
        cb += s_wave[w];
    }
    const bool any = sel[0] || sel[1] || sel[2] || sel[3];
    if (g.rank) {
#pragma unroll
        for (int k = 0, q = 0; k < SF_ITEMS; ++k) {
            if (p0 + k < g.n) g.rank[p0 + k] = sel[k] ? (int32_t)(r + q) : -1;
            q += sel[k] ? 1 : 0;
        }
    }
    if (any) {
        float d[4];
        load4<float, float4>(g.depth, p0, g.n, g.vec_depth != 0, 0.0f, d);
        double B[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) B[k] = g.inv[k];
#pragma unroll
        for (int k = 0; k < SF_ITEMS; ++k) {
            if (!sel[k]) continue;
            const uint32_t p = p0 + k;
            const uint32_t y = p / g.width, x = p - y * g.width;
            const double dd = (double)d[k];
            const double nx = (double)(2u * x + 1u) / g.fw - 1.0;
            const double ny = (double)(2u * y + 1u) / g.fh - 1.0;
            const double q0 = nx * dd, q1 = ny * dd;
            const double q2 = (g.zfar * dd) / g.zk - g.zb;
            float* row = s_xyz + 3 * (r - rb);
#pragma unroll
            for (int j = 0; j < 3; ++j) row[j] = (float)(((q0 * B[j] + q1 * B[3 + j]) + q2 * B[6 + j]) + dd * B[9 + j]);
            if (g.index) g.index[r] = (int64_t)p;
            if (g.alpha_sel) g.alpha_sel[r] = a[k];
            ++r;
        }
    }
    // the workgroup's rows are one contiguous run of xyz: written as dense dwords from LDS instead of 12-byte pieces per lane
    // (measured at 1600 x 1200, 85 % selected: 14.4 us against 20.5 us for this launch)
    __syncthreads();
    float* dst = g.xyz + 3 * (size_t)rb;
    for (uint32_t i = threadIdx.x; i < 3 * cb; i += SF_BLOCK) dst[i] = s_xyz[i];
}

// the composite: a thread takes 4 consecutive pixels of the three planes
__global__ void __launch_bounds__(SF_BLOCK)
k_surface_compose(const float* __restrict__ values, const int32_t* __restrict__ rank, const float* __restrict__ alpha,
                  const float* __restrict__ background, float* __restrict__ out, uint32_t rows, uint32_t n, int vec_in, int vec_out) {
    const uint32_t p0 = (blockIdx.x * SF_BLOCK + threadIdx.x) * SF_ITEMS;
    if (p0 >= n) return;
    float a[4]; int32_t rk[4];
    load4<float, float4>(alpha, p0, n, vec_in != 0, 0.0f, a);
    load4<int32_t, int4>(rank, p0, n, vec_in != 0, -1, rk);
    float bg[3] = {0.0f, 0.0f, 0.0f};
    if (background) { bg[0] = background[0]; bg[1] = background[1]; bg[2] = background[2]; }
    float v[3][4];
#pragma unroll
    for (int k = 0; k < SF_ITEMS; ++k) {
        const bool on = (uint32_t)rk[k] < rows;         // a negative rank is a large unsigned number
        const float* row = values + 3 * (size_t)(on ? (uint32_t)rk[k] : 0u);
        const float keep = 1.0f - a[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = (bg[c] * keep) + (on ? a[k] * row[c] : 0.0f);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* plane = out + (size_t)c * n;
        if (vec_out && p0 + 3 < n) {
            *reinterpret_cast<float4*>(plane + p0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
#pragma unroll
            for (int k = 0; k < SF_ITEMS; ++k)
                if (p0 + k < n) plane[p0 + k] = v[c][k];
        }
    }
}

inline uint32_t surface_tiles(uint32_t n) { return (n + SF_TILE - 1) / SF_TILE; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

static size_t surface_temp_bytes(int H, int W) {
    const uint32_t n = (uint32_t)H * (uint32_t)W;
    return (SF_INV_BYTES + (size_t)surface_tiles(n) * sizeof(uint32_t) + 255) & ~(size_t)255;
}

static hipError_t launch_surface_points(const TexGSSurfacePoints* p, void* temp, hipStream_t s) {
    const uint32_t n = (uint32_t)p->height * (uint32_t)p->width;
    const uint32_t tiles = surface_tiles(n);
    double* inv = (double*)temp;
    uint32_t* counts = (uint32_t*)((char*)temp + SF_INV_BYTES);
    WriteArgs g;
    g.depth = p->depth; g.alpha = p->alpha; g.inv = inv; g.offsets = counts;
    g.xyz = p->xyz; g.index = p->index; g.alpha_sel = p->alpha_sel; g.rank = p->rank;
    g.n = n; g.width = (uint32_t)p->width;
    g.vec_alpha = aligned16(p->alpha); g.vec_depth = aligned16(p->depth);
    g.thr = p->threshold;
    g.zfar = p->zfar; g.zk = p->zfar - p->znear; g.zb = (p->zfar * p->znear) / g.zk;
    g.fw = (double)p->width; g.fh = (double)p->height;
    hipLaunchKernelGGL(k_surface_count, dim3(tiles), dim3(SF_BLOCK), 0, s, p->alpha, n, g.vec_alpha, g.thr, counts);
    hipLaunchKernelGGL(k_surface_scan, dim3(1), dim3(SF_SCAN), 0, s, counts, tiles, p->count, p->full_proj, inv);
    hipLaunchKernelGGL(k_surface_write, dim3(tiles), dim3(SF_BLOCK), 0, s, g);
    return hipGetLastError();
}

static hipError_t launch_surface_compose(const TexGSSurfaceCompose* c, hipStream_t s) {
    const uint32_t n = (uint32_t)c->height * (uint32_t)c->width;
    const int vec_in = aligned16(c->alpha) && aligned16(c->rank);
    const int vec_out = aligned16(c->out) && (n % 4u == 0u);        // the planes start n floats apart
    hipLaunchKernelGGL(k_surface_compose, dim3(surface_tiles(n)), dim3(SF_BLOCK), 0, s, c->values, c->rank, c->alpha, c->background, c->out,
                       (uint32_t)c->rows, n, vec_in, vec_out);
    return hipGetLastError();
}

extern "C" {

// include/texgs_surface.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_surface_image(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return fail_msg("image size must be positive");
    if (H > TEXGS_SURFACE_MAX_SIDE || W > TEXGS_SURFACE_MAX_SIDE)
        return failf("%lld x %lld: an image side above 16384 is not supported", (long long)H, (long long)W);
    if ((long long)H * W >= (1ll << 31)) return fail_msg("image too large: height * width must be below 2^31");
    return 0;
}

size_t texgs_surface_temp_bytes(int32_t height, int32_t width) {
    return check_surface_image(height, width) ? 0 : surface_temp_bytes(height, width);
}

int texgs_surface_points(const TexGSSurfacePoints* p, void* temp, size_t temp_bytes, void* stream) {
    if (!p) return fail_msg("surface descriptor is NULL");
    if (int r = check_surface_image(p->height, p->width)) return r;
    if (!p->depth || !p->alpha || !p->full_proj || !p->xyz || !p->count || !temp)
        return fail_msg("NULL argument (depth, alpha, full_proj, xyz, count or temp)");
    if (!(p->zfar == p->zfar) || !(p->znear == p->znear) || p->zfar == p->znear) return fail_msg("zfar and znear must be two different numbers");
    if (!(p->threshold == p->threshold)) return fail_msg("threshold is NaN");
    if ((long long)p->capacity < (long long)p->height * p->width)
        return fail_msg("capacity must be at least height * width (the count is not known before the launches)");
    if (((uintptr_t)p->depth | (uintptr_t)p->alpha | (uintptr_t)p->full_proj | (uintptr_t)p->xyz | (uintptr_t)p->alpha_sel | (uintptr_t)p->rank |
         (uintptr_t)p->count) & 3)
        return fail_msg("depth, alpha, full_proj, xyz, alpha_sel, rank and count must be 4-byte aligned");
    if (((uintptr_t)p->index | (uintptr_t)temp) & 7) return fail_msg("index and temp must be 8-byte aligned");
    if (temp_bytes < surface_temp_bytes(p->height, p->width)) return fail_msg("temp is smaller than texgs_surface_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("surface_points", launch_surface_points(p, temp, s), s, false);
}

int texgs_surface_compose(const TexGSSurfaceCompose* c, void* stream) {
    if (!c) return fail_msg("compose descriptor is NULL");
    if (int r = check_surface_image(c->height, c->width)) return r;
    if (c->rows < 0) return fail_msg("rows < 0");
    if (!c->rank || !c->alpha || !c->out || (c->rows > 0 && !c->values)) return fail_msg("NULL argument (values, rank, alpha or out)");
    if (((uintptr_t)c->values | (uintptr_t)c->rank | (uintptr_t)c->alpha | (uintptr_t)c->background | (uintptr_t)c->out) & 3)
        return fail_msg("values, rank, alpha, background and out must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("surface_compose", launch_surface_compose(c, s), s, false);
}

}  // extern "C"
