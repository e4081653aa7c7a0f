// LPIPS-VGG on its own (include/texgs_lpips.h): a 3x3 convolution as an implicit GEMM on the f32-input matrix cores
// (v_mfma_f32_32x32x2_f32: exact f32 products, a k-ordered f32 chain -- the "fp32" arithmetic of uvnet.hip and mlp.hip), and the
// per-layer LPIPS head.
//
// CONVOLUTION  k_conv3x3: M = Cout, N = output pixels, K = 9 Cin; no im2col buffer anywhere.
//   A workgroup (four waves) owns 64 output channels x a tile of 8 rows x 32 columns of ONE image.  Wave w owns rows 2w, 2w + 1 of the
//   tile and both 32-channel bands: four independent 32x32 accumulators (64 registers), which is what the f32 MFMA needs to issue
//   back to back.  K runs in chunks of 8 input channels: the chunk's input tile with its one-pixel halo, [8][10][34] floats (10.6 KB),
//   is staged in LDS once -- affine, 2x2 max-pool and the zero padding are applied on that load -- and read shifted for the nine taps.
//   Within a chunk k = 8 tap + channel, so the B operand of k-step s = 4 tap + j is one word per lane at
//   [2 j + (lane >> 5)][row + dy][lane & 31 + dx]: the two 32-lane halves read two different planes, 32 consecutive words each.
//   The A operand comes straight from global memory, pre-packed by k_conv3x3_pack so that one 16-byte load per lane holds the four
//   k-steps of a tap: 18 loads per chunk.  The NEXT chunk's weights and input words are loaded into registers in front of the chunk's
//   144 MFMAs -- every load unconditional, from a clamped address, so all of them are in flight together -- and the words are
//   finished (affine, max, zero) and written to LDS behind them: the main loop waits for memory once per chunk.  The compiler is left
//   free to sink those loads into the MFMA sequence: that keeps the plain variant at 212 registers, two workgroups per CU, which
//   measured faster than pinning the loads in front of the MFMAs (339 registers, one workgroup per CU): 10.0 against 11.2 ms for an
//   800x800 pair.  Four instantiations: pool_in x affine.
//   A tile never spans two images and nothing depends on the batch size: an image's output is the same bits in any slot.
//   x and y are addressed through row / channel-plane / image strides (texgs_lpips.h; the dense ones when the descriptor's are 0).
//   The grid is (pixel tiles of an image, cout tiles, B): texgs_conv3x3 refuses 2^24 tiles or more, the launch's limit for x.
// HEAD  k_lpips_head / k_lpips_head_reduce: one thread per pixel walks the channels twice (norms, then the weighted squared
//   difference of the unit vectors) in f32 with one rounding per operation (build.py: -ffp-contract=off, so (a - b)^2 == (b - a)^2
//   and swapping the images changes no bit); the pixel sums are f64: per thread, per block (a tree in LDS), then one block per
//   pair adds the partials in a fixed order.  No atomics.
#include "common.h"
#include "lpips_checks.h"
#include "texgs_lpips.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CV_TH = TEXGS_CONV_TILE_H, CV_TW = TEXGS_CONV_TILE_W, CV_CK = TEXGS_CONV_CIN_STEP, CV_CT = TEXGS_CONV_COUT_TILE;
constexpr int CV_HH = CV_TH + 2, CV_HW = CV_TW + 2;             // the tile with its halo
constexpr int CV_PLANE = CV_HH * CV_HW;                          // words of one channel's plane in LDS
constexpr int CV_WORDS = CV_CK * CV_PLANE;                       // 2720
constexpr int CV_PRE = (CV_WORDS + 255) / 256;                   // words of a chunk per thread: 11
constexpr int CV_A_CHUNK = 2 * 9 * 64 * 4;                       // packed floats of one (cout tile, chunk): 2 bands x 9 taps x 64 lanes x 4
static_assert(CV_TH == 8 && CV_TW == 32 && CV_CK == 8 && CV_CT == 64 && TEXGS_CONV_K_STEP == 9 * CV_CK, "the kernel is written for these tiles");

int cv_chunks(int Cin) { return (Cin + CV_CK - 1) / CV_CK; }
int cv_cout_tiles(int Cout) { return (Cout + CV_CT - 1) / CV_CT; }

// pk[cout tile][chunk][band][tap][lane][j] = w[64 tile + 32 band + (lane & 31)][8 chunk + 2 j + (lane >> 5)][tap], zero outside w
__global__ void __launch_bounds__(256)
k_conv3x3_pack(const float* __restrict__ w, int Cin, int Cout, int n_chunks, int total, float* __restrict__ pk) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = idx & 3, lane = (idx >> 2) & 63;
    int rest = idx >> 8;
    const int tap = rest % 9; rest /= 9;
    const int band = rest & 1; rest >>= 1;
    const int chunk = rest % n_chunks, ct = rest / n_chunks;
    const int co = ct * CV_CT + band * 32 + (lane & 31), ci = chunk * CV_CK + 2 * j + (lane >> 5);
    pk[idx] = co < Cout && ci < Cin ? w[((size_t)co * Cin + ci) * 9 + tap] : 0.0f;
}

struct ConvArgs {
    const float* x;
    const float* pk;
    const float* bias;
    const float* in_scale;
    const float* in_shift;
    float* y;
    long long xr, xc, xi, yr, yc, yi;                            // strides in floats: row, channel plane, image
    int Cin, Cout, Ho, Wo, tiles_x, n_chunks, relu, pool;
};

// The staging of a chunk's tile is split in two so that its global loads are in flight over the MFMAs: cv_issue only loads -- from a
// clamped, always valid address, without a branch, so no load waits for another -- and cv_finish, behind the MFMAs, applies the
// affine, the 2x2 max and the zero of a word outside the (pooled) image or past Cin.
template <bool POOL>
__device__ __forceinline__ void cv_issue(const ConvArgs& a, const float* __restrict__ xb, int c, int gy, int gx, float (&raw)[POOL ? 4 : 1]) {
    const bool ok = c < a.Cin && (unsigned)gy < (unsigned)a.Ho && (unsigned)gx < (unsigned)a.Wo;
    const int cc = ok ? c : 0, yy = ok ? gy : 0, xx = ok ? gx : 0;
    const float* __restrict__ p = xb + cc * a.xc;
    if (POOL) {
        p += (2 * yy) * a.xr + 2 * xx;                          // 2 yy + 1 <= 2 Ho - 1 <= H - 1, likewise the column
        raw[0] = p[0]; raw[1] = p[1]; raw[POOL ? 2 : 0] = p[a.xr]; raw[POOL ? 3 : 0] = p[a.xr + 1];
    } else {
        raw[0] = p[yy * a.xr + xx];
    }
}

template <bool POOL, bool AFFINE>
__device__ __forceinline__ float cv_finish(const ConvArgs& a, int c, int gy, int gx, const float (&raw)[POOL ? 4 : 1]) {
    const bool ok = c < a.Cin && (unsigned)gy < (unsigned)a.Ho && (unsigned)gx < (unsigned)a.Wo;
    float v[POOL ? 4 : 1];
#pragma unroll
    for (int k = 0; k < (POOL ? 4 : 1); ++k) v[k] = raw[k];
    if (AFFINE) {
        const float sc = a.in_scale[ok ? c : 0], sh = a.in_shift[ok ? c : 0];
#pragma unroll
        for (int k = 0; k < (POOL ? 4 : 1); ++k) v[k] = v[k] * sc + sh;
    }
    const float r = POOL ? fmaxf(fmaxf(v[0], v[1]), fmaxf(v[POOL ? 2 : 0], v[POOL ? 3 : 0])) : v[0];
    return ok ? r : 0.0f;
}

template <bool POOL, bool AFFINE>
__global__ void __launch_bounds__(256)
k_conv3x3(ConvArgs a) {
    __shared__ float sm[CV_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bn = lane & 31, bk = lane >> 5;
    const int ty0 = (blockIdx.x / a.tiles_x) * CV_TH, tx0 = (blockIdx.x % a.tiles_x) * CV_TW;
    const int ct = blockIdx.y;
    const float* __restrict__ xb = a.x + blockIdx.z * a.xi;
    constexpr int NR = POOL ? 4 : 1;

    // word e of a chunk's tile: channel e / 340, halo row (e % 340) / 34, halo column e % 34 (words past 2720: a valid dummy)
    auto issue = [&](int chunk, float (&raw)[CV_PRE][NR]) {
#pragma unroll
        for (int it = 0; it < CV_PRE; ++it) {
            const int e = min(tid + 256 * it, CV_WORDS - 1);
            const int c = e / CV_PLANE, r = e - c * CV_PLANE, ry = r / CV_HW, rx = r - ry * CV_HW;
            cv_issue<POOL>(a, xb, chunk * CV_CK + c, ty0 - 1 + ry, tx0 - 1 + rx, raw[it]);
        }
    };
    auto finish = [&](int chunk, const float (&raw)[CV_PRE][NR], float (&pre)[CV_PRE]) {
#pragma unroll
        for (int it = 0; it < CV_PRE; ++it) {
            const int e = min(tid + 256 * it, CV_WORDS - 1);
            const int c = e / CV_PLANE, r = e - c * CV_PLANE, ry = r / CV_HW, rx = r - ry * CV_HW;
            pre[it] = cv_finish<POOL, AFFINE>(a, chunk * CV_CK + c, ty0 - 1 + ry, tx0 - 1 + rx, raw[it]);
        }
    };
    // the chunk's weights: one 16-byte load per (band, tap)
    auto load_a = [&](int chunk, f32x4 (&A)[2][9]) {
        const f32x4* __restrict__ pa = reinterpret_cast<const f32x4*>(a.pk + ((size_t)ct * a.n_chunks + chunk) * CV_A_CHUNK) + lane;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 9; ++t) A[b][t] = pa[(b * 9 + t) * 64];
    };

    f32x16 acc[2][2];                                            // [band][row of the wave's two]
#pragma unroll
    for (int b = 0; b < 2; ++b) { acc[b][0] = f32x16{0.f}; acc[b][1] = f32x16{0.f}; }

    float raw[CV_PRE][NR], pre[CV_PRE];
    f32x4 A[2][9], An[2][9];
    issue(0, raw);
    load_a(0, An);
    finish(0, raw, pre);
    const float* __restrict__ sb = sm + bk * CV_PLANE + (2 * wave) * CV_HW + bn;
    for (int chunk = 0; chunk < a.n_chunks; ++chunk) {
        __syncthreads();                                         // every wave has read the previous chunk's tile
#pragma unroll
        for (int it = 0; it < CV_PRE; ++it) {
            const int e = tid + 256 * it;
            if (e < CV_WORDS) sm[e] = pre[it];
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 9; ++t) A[b][t] = An[b][t];
        __syncthreads();
        const int next = chunk + 1 < a.n_chunks ? chunk + 1 : chunk;    // (the last chunk loads itself again: no branch around the loads)
        issue(next, raw);                                        // in flight over the MFMAs
        load_a(next, An);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int dy = t / 3, dx = t % 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* q = sb + (2 * j) * CV_PLANE + dy * CV_HW + dx;
                const float b0 = q[0], b1 = q[CV_HW];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[0][t][j], b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[0][t][j], b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[1][t][j], b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[1][t][j], b1, acc[1][1], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);                       // (keeps the arithmetic on the loaded words behind the MFMAs)
        finish(next, raw, pre);
    }

    // C/D layout: column = lane & 31 (the pixel), element v is channel (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of the band
    const int ox = tx0 + bn;
    if (ox >= a.Wo) return;
    float* __restrict__ yb = a.y + blockIdx.z * a.yi;
    float bias[2][16];                                           // loaded together, from a clamped index: one wait
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int v = 0; v < 16; ++v) bias[b][v] = a.bias[min(ct * CV_CT + b * 32 + (v & 3) + 8 * (v >> 2) + 4 * bk, a.Cout - 1)];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int co = ct * CV_CT + b * 32 + (v & 3) + 8 * (v >> 2) + 4 * bk;
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int oy = ty0 + 2 * wave + rr;
                float r = acc[b][rr][v] + bias[b][v];
                if (a.relu) r = fmaxf(r, 0.0f);
                if (co < a.Cout && oy < a.Ho) yb[co * a.yc + oy * a.yr + ox] = r;
            }
        }
}

// ------------------------------------------------------------------------------------------------ the head
struct HeadArgs {
    const float* f;
    const float* lin;
    double* part;                // [P][nb]
    int P, C, hw, nb;
};

// fixed-order tree over the block's 256 values; the sum is left in s[0]
__device__ __forceinline__ void lp_block_sum(double* s, int tid) {
    __syncthreads();
    for (int n = 128; n > 0; n >>= 1) {
        if (tid < n) s[tid] += s[tid + n];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_lpips_head(HeadArgs a) {
    __shared__ double s[256];
    const int tid = threadIdx.x, p = blockIdx.y;
    const size_t img = (size_t)a.C * a.hw;
    const float* __restrict__ f0 = a.f + (size_t)p * img;
    const float* __restrict__ f1 = a.f + (size_t)(a.P + p) * img;
    double sum = 0.0;
    for (long long pix = (long long)blockIdx.x * 256 + tid; pix < a.hw; pix += (long long)a.nb * 256) {
        float q0 = 0.0f, q1 = 0.0f;
        for (int c = 0; c < a.C; ++c) {
            const float u = f0[(size_t)c * a.hw + pix], v = f1[(size_t)c * a.hw + pix];
            q0 += u * u;
            q1 += v * v;
        }
        const float n0 = sqrtf(q0) + 1e-10f, n1 = sqrtf(q1) + 1e-10f;
        float d = 0.0f;
        for (int c = 0; c < a.C; ++c) {
            const float u = f0[(size_t)c * a.hw + pix] / n0, v = f1[(size_t)c * a.hw + pix] / n1;
            const float e = u - v;
            d += a.lin[c] * (e * e);
        }
        sum += (double)d;
    }
    s[tid] = sum;
    lp_block_sum(s, tid);
    if (tid == 0) a.part[(size_t)p * a.nb + blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(256)
k_lpips_head_reduce(const double* __restrict__ part, int nb, double hw, double* __restrict__ out, int layer) {
    __shared__ double s[256];
    const int tid = threadIdx.x, p = blockIdx.x;
    double sum = 0.0;
    for (int b = tid; b < nb; b += 256) sum += part[(size_t)p * nb + b];
    s[tid] = sum;
    lp_block_sum(s, tid);
    if (tid == 0) {
        double* row = out + (size_t)p * TEXGS_LPIPS_ROW;
        const double v = s[0] / hw;
        row[layer] = v;
        if (layer == TEXGS_LPIPS_LAYERS - 1) row[TEXGS_LPIPS_LAYERS] = (((row[0] + row[1]) + row[2]) + row[3]) + v;
    }
}

int lp_head_blocks(int h, int w) {
    const long long t = ((long long)h * w + 255) / 256;
    return (int)(t < TEXGS_LPIPS_HEAD_MAX_BLOCKS ? t : TEXGS_LPIPS_HEAD_MAX_BLOCKS);
}

}  // namespace

static size_t conv3x3_packed_bytes(int Cin, int Cout) { return (size_t)cv_cout_tiles(Cout) * cv_chunks(Cin) * CV_A_CHUNK * sizeof(float); }

static hipError_t launch_conv3x3_pack(const float* w, int Cin, int Cout, void* packed, hipStream_t s) {
    const int total = (int)(conv3x3_packed_bytes(Cin, Cout) / sizeof(float));           // <= 512 * 512 * 9
    hipLaunchKernelGGL(k_conv3x3_pack, dim3((total + 255) / 256), dim3(256), 0, s, w, Cin, Cout, cv_chunks(Cin), total,
                       reinterpret_cast<float*>(packed));
    return hipGetLastError();
}

static hipError_t launch_conv3x3(const TexGSConv3x3* d, hipStream_t s) {
    const int Ho = d->pool_in ? d->H / 2 : d->H, Wo = d->pool_in ? d->W / 2 : d->W;
    const int tiles_x = (Wo + CV_TW - 1) / CV_TW, tiles_y = (Ho + CV_TH - 1) / CV_TH;
    const bool xd = !d->x_row && !d->x_chan && !d->x_img, yd = !d->y_row && !d->y_chan && !d->y_img;       // dense
    const long long xr = xd ? d->W : d->x_row, xc = xd ? xr * d->H : d->x_chan, xi = xd ? xc * d->Cin : d->x_img;
    const long long yr = yd ? Wo : d->y_row, yc = yd ? yr * Ho : d->y_chan, yi = yd ? yc * d->Cout : d->y_img;
    const ConvArgs a{d->x, reinterpret_cast<const float*>(d->packed), d->bias, d->in_scale, d->in_shift, d->y, xr, xc, xi, yr, yc, yi,
                     d->Cin, d->Cout, Ho, Wo, tiles_x, cv_chunks(d->Cin), d->relu, d->pool_in};
    const dim3 grid((unsigned)(tiles_x * tiles_y), cv_cout_tiles(d->Cout), d->B);
    const bool affine = d->in_scale != nullptr;
    if (d->pool_in) {
        if (affine) hipLaunchKernelGGL((k_conv3x3<true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_conv3x3<true, false>), grid, dim3(256), 0, s, a);
    } else {
        if (affine) hipLaunchKernelGGL((k_conv3x3<false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_conv3x3<false, false>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

static size_t lpips_head_temp_bytes(int P, int h, int w) { return (size_t)P * lp_head_blocks(h, w) * sizeof(double); }

static hipError_t launch_lpips_head(const TexGSLpipsHead* d, hipStream_t s) {
    const int nb = lp_head_blocks(d->h, d->w), hw = d->h * d->w;
    const HeadArgs a{d->f, d->lin, reinterpret_cast<double*>(d->temp), d->P, d->C, hw, nb};
    hipLaunchKernelGGL(k_lpips_head, dim3(nb, d->P), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_lpips_head_reduce, dim3(d->P), dim3(256), 0, s, reinterpret_cast<const double*>(d->temp), nb, (double)hw, d->out,
                       d->layer);
    return hipGetLastError();
}

// the strides of a [B, Cn, h, w] view in floats: all zero (dense), or no two elements on one address and B img below 2^62
int check_conv_strides(const char* name, int64_t row, int64_t chan, int64_t img, int64_t B, int64_t Cn, int64_t h, int64_t w) {
    if (row == 0 && chan == 0 && img == 0) return 0;
    if (row < w || chan < 0 || img < 0 || chan / h < row || img / Cn < chan || img > (1ll << 62) / B) {
        return failf("%s_row, %s_chan, %s_img must be all 0 (dense) or row >= width, chan >= rows x row, img >= channels x chan, "
                     "B x img <= 2^62; got %lld, %lld, %lld", name, name, name, (long long)row, (long long)chan, (long long)img);
    }
    return 0;
}

int check_lpips_head_size(int32_t P, int32_t h, int32_t w) {
    if (P < 1 || P > 65535) return failf("P must be in [1,65535], got %d", (int)P);
    if (h < 1 || w < 1) return fail_msg("h and w must be at least 1");
    if ((int64_t)h * w >= (1ll << 31)) return fail_msg("map too large: h w must be below 2^31");
    return 0;
}

extern "C" {

// include/texgs_lpips.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_lpips_precision(int32_t precision) {
    if (precision == TEXGS_LPIPS_FP32) return 0;
    if (precision == TEXGS_LPIPS_BF16X3) return fail_msg("precision TEXGS_LPIPS_BF16X3 is not built into this library: use TEXGS_LPIPS_FP32");
    return failf("unknown precision %d (TEXGS_LPIPS_FP32 is 0)", (int)precision);
}

static int check_conv_channels(int32_t Cin, int32_t Cout, int32_t precision) {
    if (int r = check_lpips_precision(precision)) return r;
    if (Cin < 1 || Cin > TEXGS_CONV_MAX_CHANNELS) return failf("Cin must be in [1,512], got %d", (int)Cin);
    if (Cout < 16 || Cout > TEXGS_CONV_MAX_CHANNELS || Cout % 16) return failf("Cout must be a multiple of 16 in [16,512], got %d", (int)Cout);
    return 0;
}

size_t texgs_conv3x3_packed_bytes(int32_t Cin, int32_t Cout, int32_t precision) {
    return check_conv_channels(Cin, Cout, precision) ? 0 : conv3x3_packed_bytes(Cin, Cout);
}

int texgs_conv3x3_pack(const float* w, int32_t Cin, int32_t Cout, int32_t precision, void* packed, void* stream) {
    if (int r = check_conv_channels(Cin, Cout, precision)) return r;
    if (!w || !packed) return fail_msg("NULL argument (w or packed)");
    if ((uintptr_t)w & 3) return fail_msg("w must be 4-byte aligned");
    if ((uintptr_t)packed & 15) return fail_msg("packed must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("conv3x3_pack", launch_conv3x3_pack(w, Cin, Cout, packed, s), s, false);
}

int texgs_conv3x3(const TexGSConv3x3* d, void* stream) {
    if (!d) return fail_msg("conv descriptor is NULL");
    if (int r = check_conv_channels(d->Cin, d->Cout, d->precision)) return r;
    if ((d->relu != 0 && d->relu != 1) || (d->pool_in != 0 && d->pool_in != 1)) return fail_msg("relu and pool_in must be 0 or 1");
    if (d->B < 1 || d->B > TEXGS_CONV_MAX_BATCH) return failf("B must be in [1,65535], got %d", (int)d->B);
    if (d->H < 1 || d->W < 1) return fail_msg("H and W must be at least 1");
    const int64_t Ho = d->pool_in ? d->H / 2 : d->H, Wo = d->pool_in ? d->W / 2 : d->W;
    if (Ho < 1 || Wo < 1) return fail_msg("H and W must be at least 2 with pool_in: the pooled image would be empty");
    if ((int64_t)d->B * Ho * Wo >= (1ll << 31)) return fail_msg("too many output pixels: B Ho Wo must be below 2^31");
    const int64_t tiles = ((Wo + TEXGS_CONV_TILE_W - 1) / TEXGS_CONV_TILE_W) * ((Ho + TEXGS_CONV_TILE_H - 1) / TEXGS_CONV_TILE_H);
    if (tiles >= (1ll << 24)) return fail_msg("too many pixel tiles: an image must have fewer than 2^24 tiles of 8 x 32 output pixels");
    if (int r = check_conv_strides("x", d->x_row, d->x_chan, d->x_img, d->B, d->Cin, d->H, d->W)) return r;
    if (int r = check_conv_strides("y", d->y_row, d->y_chan, d->y_img, d->B, d->Cout, Ho, Wo)) return r;
    if (!d->x || !d->y || !d->bias) return fail_msg("NULL argument (x, y or bias)");
    if (!d->packed) return fail_msg("NULL argument (packed)");
    if ((!d->in_scale) != (!d->in_shift)) return fail_msg("in_scale and in_shift must be both NULL or both set");
    if (((uintptr_t)d->x | (uintptr_t)d->y | (uintptr_t)d->bias | (uintptr_t)d->in_scale | (uintptr_t)d->in_shift) & 3)
        return fail_msg("x, y, bias, in_scale and in_shift must be 4-byte aligned");
    if ((uintptr_t)d->packed & 15) return fail_msg("packed must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("conv3x3", launch_conv3x3(d, s), s, false);
}

size_t texgs_lpips_head_temp_bytes(int32_t P, int32_t h, int32_t w) { return check_lpips_head_size(P, h, w) ? 0 : lpips_head_temp_bytes(P, h, w); }

int texgs_lpips_head(const TexGSLpipsHead* d, void* stream) {
    if (!d) return fail_msg("head descriptor is NULL");
    if (int r = check_lpips_head_size(d->P, d->h, d->w)) return r;
    if (d->C < 1 || d->C > TEXGS_CONV_MAX_CHANNELS) return failf("C must be in [1,512], got %d", (int)d->C);
    if (d->layer < 0 || d->layer >= TEXGS_LPIPS_LAYERS) return failf("layer must be in [0,4], got %d", (int)d->layer);
    if (!d->f || !d->lin || !d->out || !d->temp) return fail_msg("NULL argument (f, lin, out or temp)");
    if (((uintptr_t)d->f | (uintptr_t)d->lin) & 3) return fail_msg("f and lin must be 4-byte aligned");
    if (((uintptr_t)d->out | (uintptr_t)d->temp) & 7) return fail_msg("out and temp must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("lpips_head", launch_lpips_head(d, s), s, false);
}

}  // extern "C"
