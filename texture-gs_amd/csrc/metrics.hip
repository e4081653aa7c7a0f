// Evaluation metrics of one view (train.py:45-93 `visualize`, utils/metrics.py): every sum that L1, PSNR, SSIM and the normal MAE
// need, in one launch over the view plus one one-block reduce.  Nothing is read back here; texgs/metrics.py finishes on the host.
//   d = image - gt            ONE fp32 subtraction (after the optional clamp to [0, 1]), as the reference subtracts; fp64 from there
//   sum |d|, sum d^2 per channel
//   SSIM as skimage.metrics.structural_similarity(channel_axis=0, data_range=1.0) defines it: uniform 7x7 window over
//        x, y, x^2, y^2, xy; cov_norm = 49/48; C1 = 0.01^2, C2 = 0.03^2;
//        S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)); the mean is over the map cropped by 3 pixels on every
//        side, so only windows wholly inside the image contribute and there is no border rule.  Window sums and the formula in fp64
//        (the product of two fp32 values is exact in fp64; the unit is built with -ffp-contract=off).
//   normal MAE (utils/metrics.py:25-37): cos = x.y / (max(|x|, 1e-6) max(|y|, 1e-6)) clamped to [-1, 1], acos in degrees, fp64;
//        numerator sum deg * alpha, denominator sum alpha (without alpha: sum deg and the pixel count)
// k_metrics: one 256-thread block per 32x32 tile, its 38x38 window (3-pixel halo) staged in LDS one channel at a time, separable
// 7-tap sums (rows into LDS as fp64, then columns); LDS 60 224 B per block, two blocks per CU.  Each block writes its NSUM partial
// sums to temp[k][block]; k_metrics_reduce (one block) adds them in a fixed order.  No atomics: a row is the same bits every run.
#include "common.h"
#include "abi_support.h"

namespace {

#define MT 32                   // tile
#define MH 3                    // halo = (7 - 1) / 2
#define MW (MT + 2 * MH)        // 38
#define NSUM 9                  // row slots 0..8 (texgs.h TEXGS_METRICS_*)

// 4 waves: butterfly inside the wave, then the four wave totals in wave order
__device__ __forceinline__ double block_sum(double v, double* s_red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    const double t = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return t;
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }       // NaN stays NaN, as torch.clamp

__global__ void __launch_bounds__(256)
k_metrics(int H, int W, int tiles_x, int nblocks, int do_clamp, const float* __restrict__ img, const float* __restrict__ gt,
          const float* __restrict__ norm, const float* __restrict__ gt_norm, const float* __restrict__ alpha,
          double* __restrict__ temp /* [NSUM][nblocks] */) {
    __shared__ float s_x[MW][MW], s_y[MW][MW];
    __shared__ double s_h[5][MW][MT];           // row sums of x, y, x^2, y^2, xy
    __shared__ double s_red[4];
    const int tile = blockIdx.x;
    const int tx0 = (tile % tiles_x) * MT, ty0 = (tile / tiles_x) * MT;
    const size_t P = (size_t)H * W;
    // this thread's pixels: column lx, rows ly0 .. ly0 + 3 of the tile
    const int lx = threadIdx.x & 31, ly0 = (threadIdx.x >> 5) * 4, px = tx0 + lx;
    double acc[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;

    for (int c = 0; c < 3; ++c) {
        const float* __restrict__ X = img + c * P;
        const float* __restrict__ Y = gt + c * P;
        __syncthreads();                                        // the previous channel's LDS reads are done
        for (int k = threadIdx.x; k < MW * MW; k += 256) {
            const int r = k / MW, q = k - r * MW, yy = ty0 + r - MH, xx = tx0 + q - MH;
            const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
            float x = 0.f, y = 0.f;                             // outside the image: read by no window that counts
            if (in) {
                x = X[(size_t)yy * W + xx]; y = Y[(size_t)yy * W + xx];
                if (do_clamp) { x = clamp01(x); y = clamp01(y); }
            }
            s_x[r][q] = x; s_y[r][q] = y;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < MW * MT; k += 256) {      // 7-tap row sums, left to right
            const int r = k / MT, q = k - r * MT;
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const double x = (double)s_x[r][q + t], y = (double)s_y[r][q + t];
                a += x; b += y; aa += x * x; bb += y * y; ab += x * y;
            }
            s_h[0][r][q] = a; s_h[1][r][q] = b; s_h[2][r][q] = aa; s_h[3][r][q] = bb; s_h[4][r][q] = ab;
        }
        __syncthreads();
        double win[5][4];                                       // 7-tap column sums, top to bottom, for the thread's four rows
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double col[10];
#pragma unroll
            for (int t = 0; t < 10; ++t) col[t] = s_h[m][ly0 + t][lx];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = 0.0;
#pragma unroll
                for (int t = 0; t < 7; ++t) v += col[j + t];
                win[m][j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int py = ty0 + ly0 + j;
            if (px >= W || py >= H) continue;
            const float d = s_x[ly0 + j + MH][lx + MH] - s_y[ly0 + j + MH][lx + MH];       // fp32, as the reference subtracts
            const double dd = (double)d;
            acc[0] += fabs(dd);
            acc[1 + c] += dd * dd;
            if (px < MH || py < MH || px >= W - MH || py >= H - MH) continue;                // the crop
            const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, cov_norm = 49.0 / 48.0;
            const double ux = win[0][j] / 49.0, uy = win[1][j] / 49.0;
            const double uxx = win[2][j] / 49.0, uyy = win[3][j] / 49.0, uxy = win[4][j] / 49.0;
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
            acc[4 + c] += (A1 * A2) / (B1 * B2);
        }
    }

    if (norm) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int py = ty0 + ly0 + j;
            if (px >= W || py >= H) continue;
            const size_t i = (size_t)py * W + px;
            const double x0 = norm[i], x1 = norm[P + i], x2 = norm[2 * P + i];
            const double y0 = gt_norm[i], y1 = gt_norm[P + i], y2 = gt_norm[2 * P + i];
            const double sx = x0 * x0 + x1 * x1 + x2 * x2, sy = y0 * y0 + y1 * y1 + y2 * y2, nx = sqrt(sx), ny = sqrt(sy);
            // |x| |y| as sqrt(sx sy) where neither norm is clamped: sqrt(s s) is s exactly, so identical normals give cos = 1 and an
            // angle of exactly 0 (sqrt(s) sqrt(s) may miss s by an ulp, which acos turns into 1e-6 degrees)
            const double den = (nx >= 1e-6 && ny >= 1e-6) ? sqrt(sx * sy) : fmax(nx, 1e-6) * fmax(ny, 1e-6);
            double cs = (x0 * y0 + x1 * y1 + x2 * y2) / den;
            cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
            const double deg = acos(cs) * (180.0 / 3.14159265358979323846);
            const double a = alpha ? (double)alpha[i] : 1.0;
            acc[7] += deg * a;
            acc[8] += a;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NSUM; ++k) {
        const double t = block_sum(acc[k], s_red);
        if (threadIdx.x == 0) temp[(size_t)k * nblocks + tile] = t;
    }
}

// One block: thread t adds the blocks t, t + 256, ... in that order; the 256 partial sums are then added pairwise in LDS
// (stride 128, 64, ... 1).  The order depends on nblocks alone.
__global__ void __launch_bounds__(256)
k_metrics_reduce(int H, int W, int nblocks, const double* __restrict__ temp, double* __restrict__ row /* [16] */) {
    __shared__ double s_p[256];
    for (int k = 0; k < NSUM; ++k) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += 256) v += temp[(size_t)k * nblocks + b];
        s_p[threadIdx.x] = v;
        __syncthreads();
        for (int s = 128; s >= 1; s >>= 1) {
            if ((int)threadIdx.x < s) s_p[threadIdx.x] += s_p[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) row[k] = s_p[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        row[TEXGS_METRICS_PIXELS] = (double)H * (double)W;
        row[TEXGS_METRICS_CROPPED] = (double)(H - 2 * MH) * (double)(W - 2 * MH);
        for (int k = TEXGS_METRICS_CROPPED + 1; k < TEXGS_METRICS_ROW; ++k) row[k] = 0.0;
    }
}

inline long long metrics_blocks(int H, int W) { return (long long)((W + MT - 1) / MT) * ((H + MT - 1) / MT); }

}  // namespace

static_assert(NSUM == TEXGS_METRICS_MAE_DEN + 1 && NSUM <= TEXGS_METRICS_PIXELS, "row layout of texgs.h");

static size_t eval_metrics_temp_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)metrics_blocks(H, W) * NSUM * sizeof(double);
}

// H, W >= 7, the tile count below 2^31 and the pointers are checked by texgs_eval_metrics below
static hipError_t launch_eval_metrics(const float* image, const float* gt_image, const float* norm, const float* gt_norm, const float* alpha, int H,
                        int W, int clamp01, void* temp, double* row, hipStream_t s) {
    const int tiles_x = (W + MT - 1) / MT, nblocks = (int)metrics_blocks(H, W);
    hipLaunchKernelGGL(k_metrics, dim3(nblocks), dim3(256), 0, s, H, W, tiles_x, nblocks, clamp01, image, gt_image, norm, gt_norm,
                       alpha, (double*)temp);
    hipLaunchKernelGGL(k_metrics_reduce, dim3(1), dim3(256), 0, s, H, W, nblocks, (const double*)temp, row);
    return hipGetLastError();
}

extern "C" {

size_t texgs_eval_metrics_temp_bytes(int32_t H, int32_t W) { return eval_metrics_temp_bytes(H, W); }

int texgs_eval_metrics(const float* image, const float* gt_image, const float* norm, const float* gt_norm, const float* alpha,
                       int32_t H, int32_t W, int32_t clamp01, void* temp, double* row, void* stream) {
    if (!image || !gt_image || !temp || !row) return fail_msg("NULL argument");
    if (H < 7 || W < 7) return fail_msg("H and W must be at least 7: the 7x7 SSIM window does not fit");
    if ((!norm) != (!gt_norm)) return fail_msg("norm and gt_norm must be both NULL or both set");
    if ((((int64_t)W + 31) / 32) * (((int64_t)H + 31) / 32) >= (1ll << 31)) return fail_msg("image too large: 2^31 tiles or more");
    hipStream_t s = (hipStream_t)stream;
    return launched("eval_metrics", launch_eval_metrics(image, gt_image, norm, gt_norm, alpha, H, W, clamp01 != 0, temp, row, s), s, false);
}

}  // extern "C"
