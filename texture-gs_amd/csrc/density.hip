// Stage-1 density control (models/gaussian3d.py:200-350, :424-462 of the reference): the per-step statistics, the plan of a
// densify_and_prune (classify, scan) and the move that writes every output row once.  Built with -ffp-contract=off: the statistics are
// compared bit for bit (sqrtf and '/' are the correctly rounded ones here; __fsqrt_rn is NOT: this toolchain maps it to the native
// approximation).  No global atomics and no workgroup waits on another: the scan is three plain launches.
#include "common.h"
#include "abi_support.h"

namespace {

constexpr int DN_BLOCK = 256;
constexpr int DN_ITEMS = 4;                         // Gaussians per thread in the plan kernels
constexpr int DN_TILE = DN_BLOCK * DN_ITEMS;        // Gaussians one scan block covers (1024)
constexpr int DN_CH = 4;                            // scanned counts: kept, clone, split parent, surviving child pair

// ---- per-step statistics: one thread owns one Gaussian ----
__global__ void __launch_bounds__(DN_BLOCK)
k_density_stats(const float* __restrict__ grad, const int32_t* __restrict__ radii, uint32_t n, float* __restrict__ accum,
                float* __restrict__ denom, float* __restrict__ max_radii) {
    const uint32_t i = blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    const float gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
    max_radii[i] = fmaxf(max_radii[i], (float)r);
}

// ---- plan ----
struct PlanArgs {
    const float* accum; const float* denom; const float* scaling; const float* opacity;
    uint32_t n;
    float max_grad, min_opacity, dense_scale, big_scale;
    int densify, use_big;
};

__device__ __forceinline__ uint32_t classify(const PlanArgs& a, uint32_t i) {
    const float s0 = expf(a.scaling[3 * (size_t)i]), s1 = expf(a.scaling[3 * (size_t)i + 1]), s2 = expf(a.scaling[3 * (size_t)i + 2]);
    const float m = fmaxf(fmaxf(s0, s1), s2);
    const float x = a.opacity[i];
    const float o = 1.0f / (1.0f + expf(-x));
    const bool low = o < a.min_opacity;
    bool clone = false, split = false;
    if (a.densify) {
        float g = (a.accum[i] / a.denom[i]);
        if (g != g) g = 0.0f;
        const bool small = m <= a.dense_scale;
        clone = (sqrtf(g * g) >= a.max_grad) && small;      // torch.norm of one element, gaussian3d.py:305
        split = (g >= a.max_grad) && !small;                     // the padded gradient itself, :283
    }
    uint32_t act = 0;
    if (split) {
        act |= TEXGS_DENSITY_SPLIT;
        const float c0 = expf(logf(s0 / 1.6f)), c1 = expf(logf(s1 / 1.6f)), c2 = expf(logf(s2 / 1.6f));
        const float mc = fmaxf(fmaxf(c0, c1), c2);
        if (!(low || (a.use_big && mc > a.big_scale))) act |= TEXGS_DENSITY_CHILD;
    } else {
        const bool keep = !(low || (a.use_big && m > a.big_scale));     // a clone shares its parent's values, so its fate
        if (keep) act |= TEXGS_DENSITY_KEEP;
        if (clone) act |= keep ? (TEXGS_DENSITY_CLONE | TEXGS_DENSITY_CLONE_KEPT) : TEXGS_DENSITY_CLONE;
    }
    return act;
}

// the four 0/1 counts of an action, 16 bits each (a tile's sums stay below 2^16)
__device__ __forceinline__ unsigned long long counts_of(uint32_t act) {
    return (unsigned long long)((act & TEXGS_DENSITY_KEEP) ? 1 : 0)
         | ((unsigned long long)((act & TEXGS_DENSITY_CLONE_KEPT) ? 1 : 0) << 16)
         | ((unsigned long long)((act & TEXGS_DENSITY_SPLIT) ? 1 : 0) << 32)
         | ((unsigned long long)((act & TEXGS_DENSITY_CHILD) ? 1 : 0) << 48);
}

// exclusive scan of one packed value per thread over the block; *total = the block's sum (every thread gets it)
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long* total) {
    __shared__ unsigned long long s_wave[DN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < DN_BLOCK / 64; ++w) {
        const unsigned long long t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// launch 1: action bytes and per-tile counts
__global__ void __launch_bounds__(DN_BLOCK)
k_density_classify(PlanArgs a, uint8_t* __restrict__ action, uint32_t* __restrict__ tile_counts) {
    const uint32_t base = blockIdx.x * DN_TILE + threadIdx.x * DN_ITEMS;
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < DN_ITEMS; ++k) {
        const uint32_t i = base + k;
        if (i < a.n) {
            const uint32_t act = classify(a, i);
            action[i] = (uint8_t)act;
            mine += counts_of(act);
        }
    }
    unsigned long long total;
    (void)block_exclusive(mine, &total);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < DN_CH; ++c) tile_counts[DN_CH * (size_t)blockIdx.x + c] = (uint32_t)((total >> (16 * c)) & 0xFFFFu);
    }
}

// launch 2: ONE block turns the tile counts into exclusive offsets, DN_BLOCK tiles per pass with a running carry; totals[c] = the sums
__global__ void __launch_bounds__(DN_BLOCK)
k_density_scan_tiles(uint32_t* __restrict__ tile_counts, uint32_t tiles, uint32_t* __restrict__ totals) {
    __shared__ uint32_t s_wave[DN_BLOCK / 64][DN_CH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry[DN_CH] = {0, 0, 0, 0};
    for (uint32_t first = 0; first < tiles; first += DN_BLOCK) {
        const uint32_t t = first + threadIdx.x;
        uint32_t v[DN_CH], inc[DN_CH];
#pragma unroll
        for (int c = 0; c < DN_CH; ++c) {
            v[c] = t < tiles ? tile_counts[DN_CH * (size_t)t + c] : 0u;
            inc[c] = v[c];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(inc[c], d, 64);
                if (lane >= d) inc[c] += up;
            }
            if (lane == 63) s_wave[wave][c] = inc[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < DN_CH; ++c) {
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < DN_BLOCK / 64; ++w) {
                const uint32_t s = s_wave[w][c];
                if (w < wave) before += s;
                all += s;
            }
            if (t < tiles) tile_counts[DN_CH * (size_t)t + c] = carry[c] + before + inc[c] - v[c];
            carry[c] += all;
        }
        __syncthreads();
    }
    if (threadIdx.x < DN_CH) totals[threadIdx.x] = carry[threadIdx.x];
}

// launch 3: per-tile scan plus the tile's offset -> rank[c][i], the exclusive count over all i' < i
__global__ void __launch_bounds__(DN_BLOCK)
k_density_ranks(const uint8_t* __restrict__ action, uint32_t n, const uint32_t* __restrict__ tile_offsets, int32_t* __restrict__ rank) {
    const uint32_t base = blockIdx.x * DN_TILE + threadIdx.x * DN_ITEMS;
    uint32_t act[DN_ITEMS];
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < DN_ITEMS; ++k) {
        act[k] = base + k < n ? action[base + k] : 0u;
        mine += counts_of(act[k]);
    }
    unsigned long long total;
    unsigned long long run = block_exclusive(mine, &total);
    uint32_t off[DN_CH];
#pragma unroll
    for (int c = 0; c < DN_CH; ++c) off[c] = tile_offsets[DN_CH * (size_t)blockIdx.x + c];
#pragma unroll
    for (int k = 0; k < DN_ITEMS; ++k) {
        const uint32_t i = base + k;
        if (i < n) {
#pragma unroll
            for (int c = 0; c < DN_CH; ++c)
                rank[(size_t)c * n + i] = (int32_t)(off[c] + (uint32_t)((run >> (16 * c)) & 0xFFFFu));
        }
        run += counts_of(act[k]);
    }
}

// ---- move ----
constexpr int DN_MAX_ROWS = TEXGS_DENSITY_MAX_ROWS;

struct MoveArgs {
    TexGSDensityRow row[DN_MAX_ROWS];
    uint32_t first_block[DN_MAX_ROWS + 1];      // blocks [first_block[d], first_block[d+1]) work on row[d]
    int rows;
    uint32_t n;
    const uint8_t* action; const int32_t* rank;
    uint32_t n_kept, n_clone, n_split, n_child;
    const float* scaling; const float* rotation; const float* noise;      // sources of the children's positions
};

// utils/general.py:87-108 row `w` of R(q / |q|) times v
__device__ __forceinline__ float rotate_row(const float* __restrict__ q4, int w, float v0, float v1, float v2) {
    const float a = q4[0], b = q4[1], c = q4[2], d = q4[3];
    const float norm = sqrtf(a * a + b * b + c * c + d * d);
    const float r = (a / norm), x = (b / norm), y = (c / norm), z = (d / norm);
    float m0, m1, m2;
    if (w == 0)      { m0 = 1.0f - 2.0f * (y * y + z * z); m1 = 2.0f * (x * y - r * z);        m2 = 2.0f * (x * z + r * y); }
    else if (w == 1) { m0 = 2.0f * (x * y + r * z);        m1 = 1.0f - 2.0f * (x * x + z * z); m2 = 2.0f * (y * z - r * x); }
    else             { m0 = 2.0f * (x * z - r * y);        m1 = 2.0f * (y * z + r * x);        m2 = 1.0f - 2.0f * (x * x + y * y); }
    return (m0 * v0 + m1 * v1) + m2 * v2;
}

// One thread per float of a SOURCE tensor: (i, w) = Gaussian and column.  It writes that float to each output row the Gaussian has
// (kept original, clone, two children); lanes that share a row write consecutive floats of it.
__global__ void __launch_bounds__(DN_BLOCK)
k_density_move(MoveArgs a) {
    int d = 0;
    while (d + 1 < a.rows && blockIdx.x >= a.first_block[d + 1]) ++d;
    const TexGSDensityRow R = a.row[d];
    const uint32_t width = (uint32_t)R.width;
    const unsigned long long flat = (unsigned long long)(blockIdx.x - a.first_block[d]) * DN_BLOCK + threadIdx.x;
    const unsigned long long count = (unsigned long long)a.n * width;
    if (flat >= count) return;
    uint32_t i, w;
    if (count <= 0xFFFFFFFFull) { i = (uint32_t)flat / width; w = (uint32_t)flat - i * width; }
    else { i = (uint32_t)(flat / width); w = (uint32_t)(flat - (unsigned long long)i * width); }
    const uint32_t act = a.action[i];
    if (!(act & (TEXGS_DENSITY_KEEP | TEXGS_DENSITY_CLONE_KEPT | TEXGS_DENSITY_CHILD))) return;
    const float v = R.src[flat];
    const bool moment = R.kind == TEXGS_DENSITY_ROW_MOMENT;
    if (act & TEXGS_DENSITY_KEEP)
        R.dst[(size_t)(uint32_t)a.rank[i] * width + w] = v;
    if (act & TEXGS_DENSITY_CLONE_KEPT)
        R.dst[((size_t)a.n_kept + (uint32_t)a.rank[(size_t)a.n + i]) * width + w] = moment ? 0.0f : v;
    if (act & TEXGS_DENSITY_CHILD) {
        const size_t r0 = (size_t)a.n_kept + a.n_clone + (uint32_t)a.rank[3 * (size_t)a.n + i];
        const size_t r1 = r0 + a.n_child;
        float c0 = v, c1 = v;
        if (moment) {
            c0 = c1 = 0.0f;
        } else if (R.kind == TEXGS_DENSITY_ROW_SCALING) {
            c0 = c1 = logf(expf(v) / 1.6f);                 // log(s / (0.8 * 2)), gaussian3d.py:292
        } else if (R.kind == TEXGS_DENSITY_ROW_XYZ) {
            const uint32_t j = (uint32_t)a.rank[2 * (size_t)a.n + i];          // rank among ALL split parents: the noise row
            const float s0 = expf(a.scaling[3 * (size_t)i]), s1 = expf(a.scaling[3 * (size_t)i + 1]), s2 = expf(a.scaling[3 * (size_t)i + 2]);
            const float* e0 = a.noise + 3 * (size_t)j;
            const float* e1 = a.noise + 3 * ((size_t)a.n_split + j);
            const float* q = a.rotation + 4 * (size_t)i;
            c0 = rotate_row(q, (int)w, s0 * e0[0], s1 * e0[1], s2 * e0[2]) + v;
            c1 = rotate_row(q, (int)w, s0 * e1[0], s1 * e1[1], s2 * e1[2]) + v;
        }
        R.dst[r0 * width + w] = c0;
        R.dst[r1 * width + w] = c1;
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

static hipError_t launch_density_stats(const float* grad, const int32_t* radii, int n, float* accum, float* denom, float* max_radii, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_density_stats, dim3(((uint32_t)n + DN_BLOCK - 1) / DN_BLOCK), dim3(DN_BLOCK), 0, s, grad, radii, (uint32_t)n, accum,
                       denom, max_radii);
    return hipGetLastError();
}

static size_t density_plan_temp_bytes(int n) {
    const size_t tiles = ((size_t)(n > 0 ? n : 1) + DN_TILE - 1) / DN_TILE;
    return align256(tiles * DN_CH * sizeof(uint32_t));
}

static hipError_t launch_density_plan(const TexGSDensityPlan* p, uint8_t* action, int32_t* rank, uint32_t* totals, void* temp, hipStream_t s) {
    const uint32_t n = (uint32_t)p->n;
    if (n == 0) return hipMemsetAsync(totals, 0, DN_CH * sizeof(uint32_t), s);
    const uint32_t tiles = (n + DN_TILE - 1) / DN_TILE;
    PlanArgs a;
    a.accum = p->accum; a.denom = p->denom; a.scaling = p->scaling; a.opacity = p->opacity; a.n = n;
    a.max_grad = p->max_grad; a.min_opacity = p->min_opacity; a.dense_scale = p->dense_scale; a.big_scale = p->big_scale;
    a.densify = p->densify; a.use_big = p->use_big;
    uint32_t* tile_counts = (uint32_t*)temp;
    hipLaunchKernelGGL(k_density_classify, dim3(tiles), dim3(DN_BLOCK), 0, s, a, action, tile_counts);
    hipLaunchKernelGGL(k_density_scan_tiles, dim3(1), dim3(DN_BLOCK), 0, s, tile_counts, tiles, totals);
    hipLaunchKernelGGL(k_density_ranks, dim3(tiles), dim3(DN_BLOCK), 0, s, (const uint8_t*)action, n, (const uint32_t*)tile_counts, rank);
    return hipGetLastError();
}

static hipError_t launch_density_move(const TexGSDensityMove* m, hipStream_t s) {
    MoveArgs a;
    unsigned long long blocks = 0;
    for (int d = 0; d < m->rows; ++d) {
        a.row[d] = m->row[d];
        a.first_block[d] = (uint32_t)blocks;
        blocks += ((unsigned long long)(uint32_t)m->n * (uint32_t)m->row[d].width + DN_BLOCK - 1) / DN_BLOCK;
        if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    }
    for (int d = m->rows; d <= DN_MAX_ROWS; ++d) a.first_block[d] = (uint32_t)blocks;
    for (int d = m->rows; d < DN_MAX_ROWS; ++d) a.row[d] = TexGSDensityRow{nullptr, nullptr, 1, TEXGS_DENSITY_ROW_COPY};
    a.rows = m->rows; a.n = (uint32_t)m->n; a.action = m->action; a.rank = m->rank;
    a.n_kept = (uint32_t)m->n_kept; a.n_clone = (uint32_t)m->n_clone; a.n_split = (uint32_t)m->n_split; a.n_child = (uint32_t)m->n_child;
    a.scaling = m->scaling; a.rotation = m->rotation; a.noise = m->noise;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_density_move, dim3((uint32_t)blocks), dim3(DN_BLOCK), 0, s, a);
    return hipGetLastError();
}

extern "C" {

int texgs_density_stats(const float* grad, const int32_t* radii, int32_t n, float* accum, float* denom, float* max_radii, void* stream) {
    if (n < 0) return fail_msg("n < 0");
    if (n > 0 && (!grad || !radii || !accum || !denom || !max_radii)) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("density_stats", launch_density_stats(grad, radii, n, accum, denom, max_radii, s), s, false);
}

size_t texgs_density_plan_temp_bytes(int32_t n) { return density_plan_temp_bytes(n); }

int texgs_density_plan(const TexGSDensityPlan* plan, uint8_t* action, int32_t* rank, uint32_t* totals, void* temp, void* stream) {
    if (!plan || !totals) return fail_msg("NULL argument");
    if (plan->n < 0) return fail_msg("n < 0");
    if (plan->n > 0 && (!plan->scaling || !plan->opacity || !action || !rank || !temp)) return fail_msg("NULL argument");
    if (plan->n > 0 && plan->densify && (!plan->accum || !plan->denom)) return fail_msg("accum and denom are required to densify");
    if (plan->densify && !(plan->max_grad > 0.0f)) return fail_msg("max_grad must be positive (with 0 the reference splits its own clones)");
    hipStream_t s = (hipStream_t)stream;
    return launched("density_plan", launch_density_plan(plan, action, rank, totals, temp, s), s, false);
}

int texgs_density_move(const TexGSDensityMove* m, void* stream) {
    if (!m) return fail_msg("NULL argument");
    if (m->n < 0 || m->n_kept < 0 || m->n_clone < 0 || m->n_split < 0 || m->n_child < 0) return fail_msg("negative count");
    if (m->n_kept > m->n || m->n_clone > m->n || m->n_split > m->n || m->n_child > m->n_split) return fail_msg("totals exceed n");
    if ((int64_t)m->n_kept + m->n_clone + 2ll * m->n_child >= (1ll << 31)) return fail_msg("the new row count reaches 2^31");
    if (m->rows < 0 || m->rows > TEXGS_DENSITY_MAX_ROWS) return fail_msg("rows must be in [0, TEXGS_DENSITY_MAX_ROWS]");
    if (m->n == 0 || m->rows == 0) return 0;
    if (!m->action || !m->rank) return fail_msg("NULL argument");
    const bool out_rows = m->n_kept + m->n_clone + m->n_child > 0;
    for (int d = 0; d < m->rows; ++d) {
        const TexGSDensityRow& r = m->row[d];
        if (r.width < 1) return fail_msg("row width < 1");
        if (r.kind < TEXGS_DENSITY_ROW_COPY || r.kind > TEXGS_DENSITY_ROW_XYZ) return fail_msg("unknown row kind");
        if (r.kind == TEXGS_DENSITY_ROW_XYZ && r.width != 3) return fail_msg("an XYZ row has width 3");
        if (!r.src || (out_rows && !r.dst)) return fail_msg("NULL row pointer");
        if (r.kind == TEXGS_DENSITY_ROW_XYZ && m->n_child > 0 && (!m->scaling || !m->rotation || !m->noise))
            return fail_msg("an XYZ row with children needs scaling, rotation and noise");
    }
    if (!out_rows) return 0;        // everything pruned: there is no row to write
    return launched("density_move", launch_density_move(m, (hipStream_t)stream), (hipStream_t)stream, false);
}

}  // extern "C"
