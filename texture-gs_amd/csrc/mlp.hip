// A bias-free ReLU MLP of width 128 on its own (include/texgs_mlp.h): what tiny-cuda-nn's Network(n_in, n_out, "FullyFusedMLP") computes,
// forward and backward, on the f32-input matrix cores (v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulation -- the "fp32"
// arithmetic of uvnet.hip; no bf16 here).
//
//     xp  = [x | 1 ... 1]                                    n_in columns of x, pin - n_in columns of ones   (pin = pad16(n_in))
//     h_1 = relu(W_1 xp);  h_k = relu(W_k h_{k-1});  y = (W_out h_L)[:n_out]          L = 1 or 2 hidden layers
//     params = W_1 [128, pin] | L - 1 x [128, 128] | W_out [pout, 128], row-major, back to back          (pout = pad16(n_out))
//
// Both kernels are uvnet.hip's shapes made general.  A workgroup is four waves; wave w owns output rows [32 w, 32 w + 32) of every
// layer and holds its 32 x 128 slice of the layer's matrix in 64 VGPRs as the MFMA's A operand; the B operand is a tile of points in
// LDS, k-major ([neuron][point]), read one word per lane -- the two 32-lane halves read two different rows, so any pitch is
// conflict-free for the GEMMs; the pitches are odd (129 / 65) for the accesses that run ACROSS rows (the tiles' transposed
// loads and stores, the point-major reads of the weight-gradient products).
//
// k_mlp_pack re-packs every matrix a call needs into A-operand order, each as a zero-padded 128 x 128 (64 KB), into the caller's
// temp memory on the call's stream.  A matrix with fewer than 128 columns runs fewer k-steps (in chunks of 8 steps = 16 columns:
// pin and pout are multiples of 16), one with fewer than 128 rows runs on fewer waves.
//
// FORWARD  k_mlp_forward: one launch, one workgroup per 128 points, ONE activation plane [128][129] in LDS (66 KB, two workgroups per CU)
//   that every layer reads, then -- behind a barrier -- overwrites.  The input tile is transposed into it (x rows are read as scalars:
//   they are not 16-byte aligned when n_in = 3), the output tile is transposed out of it, so global accesses are contiguous.
// BACKWARD k_mlp_backward: a persistent grid of <= 256 workgroups, 64 points per tile, four planes [128][65] in LDS (133 KB):
//     sX = xp, sD = dy (rows >= n_out zero), sH1 / sHL = the recomputed activations
//     d_L = (W_out^T dy) . [h_L > 0]  -> overwrites h_L         dW_out += dy h_L^T
//     d_1 = (W_2^T d_2) . [h_1 > 0]   -> overwrites h_1         dW_2   += d_2 h_1^T                   (L = 2)
//     dx  = (W_1^T d_1)[:n_in]        -> staged in sD           dW_1   += d_1 xp^T
//   (the ones columns of xp make the padded columns of dW_1 the sums of d_1, each by the same instruction sequence: equal bit for bit).
//   The three weight gradients stay in registers (192 VGPRs) across a workgroup's tiles; each workgroup writes its partial sums once,
//   k_mlp_backward_reduce adds them in workgroup order.  No atomics: two calls give the same bits.
#include "common.h"
#include "abi_support.h"
#include "texgs_mlp.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int ML_H = TEXGS_MLP_WIDTH;
constexpr int ML_FT = TEXGS_MLP_FORWARD_TILE, ML_FP = ML_FT + 1;
constexpr int ML_BT = TEXGS_MLP_BACKWARD_TILE, ML_BP = ML_BT + 1;
constexpr int ML_MAT = ML_H * ML_H;                    // floats of one packed (or partial) matrix
constexpr int ML_MAT_BYTES = ML_MAT * 4;
constexpr int ML_FWD_MATS = 3;                         // W_1, W_2, W_out
constexpr int ML_BWD_MATS = 5;                         // W_1, W_2, W_out^T, W_2^T, W_1^T
static_assert(ML_H == 128 && ML_FT == 128 && ML_BT == 64, "the kernels are written for these tiles");

// One packed matrix M [128 x 128]: trans == 0: M[r][k] = src[r][k] of the row-major src [rows][cols] at params + off;
// trans == 1: M[r][k] = src[k][r].  Zero outside src; rows == 0: an unused slot (all zero).
struct MlpPackMat { int off, rows, cols, trans; };
struct MlpPackArgs { MlpPackMat m[ML_BWD_MATS]; };

// A-operand order of mfma_f32_32x32x2f32, four k-steps per 16-byte load (k_uv_pack_bwd's):
//   pk[m][band][g][lane][j] = M_m[32 band + (lane & 31)][2 (4 g + j) + (lane >> 5)]
__global__ void __launch_bounds__(256)
k_mlp_pack(const float* __restrict__ params, MlpPackArgs a, int n_mat, float* __restrict__ pk) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_mat * ML_MAT) return;
    const int j = idx & 3, lane = (idx >> 2) & 63, g = (idx >> 8) & 15, band = (idx >> 12) & 3, m = idx >> 14;
    const int r = band * 32 + (lane & 31), k = 2 * (4 * g + j) + (lane >> 5);
    const MlpPackMat mm = a.m[m];
    float v = 0.0f;
    if (mm.trans == 0) { if (r < mm.rows && k < mm.cols) v = params[mm.off + r * mm.cols + k]; }
    else { if (k < mm.rows && r < mm.cols) v = params[mm.off + k * mm.cols + r]; }
    pk[idx] = v;
}

// One wave's 32 x 128 slice of packed matrix `mat`: buffer loads, the descriptor and the slice's byte offset are scalars
__device__ __forceinline__ void mlp_load_a(float (&A)[64], __amdgpu_buffer_rsrc_t rsrc, int mat, int wave, int lane) {
    const int slice_bytes = (mat * 4 + wave) * (16 * 64 * 16);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 16, slice_bytes + g * 1024, 0);
        A[4 * g] = __uint_as_float(v.x); A[4 * g + 1] = __uint_as_float(v.y); A[4 * g + 2] = __uint_as_float(v.z); A[4 * g + 3] = __uint_as_float(v.w);
    }
}

// c[wave's 32 rows x 32 NB points] += A (in registers) x sIn[16 n_chunks rows][32 NB points]; n_chunks is uniform
template <int NB, int PITCH>
__device__ __forceinline__ void mlp_gemm(const float (&A)[64], const float (*sIn)[PITCH], int n_chunks, int bn, int bk, f32x16 (&c)[NB]) {
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        if (ch < n_chunks) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int s = 8 * ch + q;
                const float* row = &sIn[2 * s + bk][bn];
#pragma unroll
                for (int t = 0; t < NB; ++t) c[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[s], row[32 * t], c[t], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);       // (keeps the scheduler from hoisting every LDS read of the layer)
        }
    }
}

// C/D layout: col = lane & 31, element v is row (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of the wave's 32
__device__ __forceinline__ int mlp_row(int wave, int bk, int v) { return wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * bk; }

template <int NB, int PITCH, bool RELU>
__device__ __forceinline__ void mlp_store(float (*sOut)[PITCH], int wave, int bn, int bk, const f32x16 (&c)[NB]) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int i = mlp_row(wave, bk, v);
#pragma unroll
        for (int t = 0; t < NB; ++t) sOut[i][32 * t + bn] = RELU ? fmaxf(c[t][v], 0.0f) : c[t][v];
    }
}

// rows [0, n) of a plane <- the tile's rows of a row-major global [N][n] (zero past N); rows [n, n_pad) <- fill; rows [n_pad, n_rows) <- 0
template <int TILE, int PITCH>
__device__ __forceinline__ void mlp_load_tile(float (*sm)[PITCH], const float* __restrict__ src, size_t p0, size_t N, int n, int n_pad, int n_rows,
                                              float fill, int tid) {
    const size_t base = p0 * (size_t)n, total = N * (size_t)n;
    for (int e = tid; e < n * TILE; e += 256) {
        const int p = e / n, c = e - p * n;
        sm[c][p] = base + e < total ? src[base + e] : 0.0f;
    }
    for (int e = tid; e < (n_rows - n) * TILE; e += 256) {
        const int r = n + e / TILE, p = e % TILE;
        sm[r][p] = r < n_pad ? fill : 0.0f;
    }
}

// the tile's rows of a row-major global [N][n] <- rows [0, n) of a plane
template <int TILE, int PITCH>
__device__ __forceinline__ void mlp_store_tile(const float (*sm)[PITCH], float* __restrict__ dst, size_t p0, size_t N, int n, int tid) {
    const size_t base = p0 * (size_t)n, total = N * (size_t)n;
    for (int e = tid; e < n * TILE; e += 256) {
        const int p = e / n, c = e - p * n;
        if (base + e < total) dst[base + e] = sm[c][p];
    }
}

struct MlpFwdArgs {
    const float* pk;                 // W_1, W_2 (unused slot when L = 1), W_out
    const float* x;
    float* y;
    int N, n_in, n_out, pin, pout, L;
};

__global__ void __launch_bounds__(256, 2)
k_mlp_forward(MlpFwdArgs a) {
    __shared__ float sm[ML_H][ML_FP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bn = lane & 31, bk = lane >> 5;
    const size_t p0 = (size_t)blockIdx.x * ML_FT;
    mlp_load_tile<ML_FT, ML_FP>(sm, a.x, p0, (size_t)a.N, a.n_in, a.pin, a.pin, 1.0f, tid);
    const __amdgpu_buffer_rsrc_t pk = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.pk), 0, ML_FWD_MATS * ML_MAT_BYTES, 0x00020000);
    float A[64];
    mlp_load_a(A, pk, 0, wave, lane);
    __syncthreads();
    for (int layer = 0; layer < a.L; ++layer) {
        f32x16 c[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) c[t] = f32x16{0.f};
        mlp_gemm<4, ML_FP>(A, sm, layer == 0 ? a.pin / 16 : 8, bn, bk, c);
        mlp_load_a(A, pk, layer + 1 < a.L ? layer + 1 : 2, wave, lane);       // the next layer's slice, in flight over the epilogue
        __syncthreads();                                                      // every wave has read the layer's input
        mlp_store<4, ML_FP, true>(sm, wave, bn, bk, c);
        __syncthreads();
    }
    // ---- output layer on the bands pout needs
    const int bands = (a.pout + 31) / 32;
    f32x16 c[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c[t] = f32x16{0.f};
    if (wave < bands) mlp_gemm<4, ML_FP>(A, sm, 8, bn, bk, c);
    __syncthreads();
    if (wave < bands) mlp_store<4, ML_FP, false>(sm, wave, bn, bk, c);
    __syncthreads();
    mlp_store_tile<ML_FT, ML_FP>(sm, a.y, p0, (size_t)a.N, a.n_out, tid);
}

// ------------------------------------------------------------------------------------------------ backward
typedef float BwPlane[ML_BP];

// dW[wave's 32 rows x 32 n_blocks] += sD[rows][64 points] x sH[32 n_blocks rows][64 points]^T, k = the point
__device__ __forceinline__ void mlp_outer(const BwPlane* sD, const BwPlane* sH, int wave, int n_blocks, int bn, int bk, f32x16 (&dW)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t < n_blocks) {
#pragma unroll
            for (int s = 0; s < ML_BT / 2; ++s) {
                dW[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(sD[32 * wave + bn][2 * s + bk], sH[32 * t + bn][2 * s + bk], dW[t], 0, 0, 0);
                if ((s & 7) == 7) __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// d = c . [h > 0], in place of h
__device__ __forceinline__ void mlp_mask_into(BwPlane* sH, int wave, int bn, int bk, const f32x16 (&c)[2]) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int i = mlp_row(wave, bk, v);
        sH[i][bn] = sH[i][bn] > 0.0f ? c[0][v] : 0.0f;
        sH[i][32 + bn] = sH[i][32 + bn] > 0.0f ? c[1][v] : 0.0f;
    }
}

struct MlpBwdArgs {
    const float* pk;                 // W_1, W_2, W_out^T, W_2^T, W_1^T (the W_2 slots unused when L = 1)
    const float* x;
    const float* dy;
    float* dx;                       // NULL: not wanted
    float* partW;                    // [grid][3][128][128]: dW_1, dW_2, dW_out; NULL: d_params not wanted
    int N, n_tiles, n_in, n_out, pin, pout, L;
};

__global__ void __launch_bounds__(256, 1)
k_mlp_backward(MlpBwdArgs a) {
    __shared__ float sX[ML_H][ML_BP], sH1[ML_H][ML_BP], sHL[ML_H][ML_BP], sD[ML_H][ML_BP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bn = lane & 31, bk = lane >> 5;
    const int bands_in = (a.pin + 31) / 32, bands_out = (a.pout + 31) / 32;
    const bool want_dp = a.partW != nullptr, want_dx = a.dx != nullptr, two = a.L == 2;
    const __amdgpu_buffer_rsrc_t pk = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.pk), 0, ML_BWD_MATS * ML_MAT_BYTES, 0x00020000);

    f32x16 dW1[4], dW2[4], dWo[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { dW1[t] = f32x16{0.f}; dW2[t] = f32x16{0.f}; dWo[t] = f32x16{0.f}; }
    float A[64];

    // one layer of the recomputed forward: sOut = relu(M_mat sIn)
    auto forward_layer = [&](int mat, const BwPlane* sIn, int n_chunks, BwPlane* sOut) {
        f32x16 c[2] = {f32x16{0.f}, f32x16{0.f}};
        mlp_load_a(A, pk, mat, wave, lane);
        mlp_gemm<2, ML_BP>(A, sIn, n_chunks, bn, bk, c);
        mlp_store<2, ML_BP, true>(sOut, wave, bn, bk, c);
        __syncthreads();
    };
    // one layer of the chain: dW += sDin sH^T (this wave's rows, if it has any), then sH <- (M_mat sDin) . [sH > 0]
    auto backward_layer = [&](int mat, const BwPlane* sDin, int n_chunks, BwPlane* sH, bool rows_here, f32x16 (&dW)[4]) {
        f32x16 c[2] = {f32x16{0.f}, f32x16{0.f}};
        mlp_load_a(A, pk, mat, wave, lane);
        mlp_gemm<2, ML_BP>(A, sDin, n_chunks, bn, bk, c);
        if (want_dp && rows_here) mlp_outer(sDin, sH, wave, 4, bn, bk, dW);
        __syncthreads();                         // every wave has read sH
        mlp_mask_into(sH, wave, bn, bk, c);
        __syncthreads();
    };
    // the first layer: dW_1 += d_1 xp^T on the column blocks pin needs; dx = W_1^T d_1 on the bands pin needs, staged in sD
    auto first_layer = [&](const BwPlane* sD1) {
        if (want_dp) mlp_outer(sD1, sX, wave, bands_in, bn, bk, dW1);
        if (want_dx) {
            if (wave < bands_in) {
                f32x16 c[2] = {f32x16{0.f}, f32x16{0.f}};
                mlp_load_a(A, pk, 4, wave, lane);
                mlp_gemm<2, ML_BP>(A, sD1, 8, bn, bk, c);
                mlp_store<2, ML_BP, false>(sD, wave, bn, bk, c);      // (dy was last read two barriers ago)
            }
        }
    };

    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const size_t p0 = (size_t)tile * ML_BT;
        // ---- the tile's inputs; points past N get dy = 0 and add nothing anywhere
        mlp_load_tile<ML_BT, ML_BP>(sX, a.x, p0, (size_t)a.N, a.n_in, a.pin, 32 * bands_in, 1.0f, tid);
        mlp_load_tile<ML_BT, ML_BP>(sD, a.dy, p0, (size_t)a.N, a.n_out, a.n_out, 32 * bands_out, 0.0f, tid);
        __syncthreads();
        if (two) {
            forward_layer(0, sX, a.pin / 16, sH1);
            forward_layer(1, sH1, 8, sHL);
        } else {
            forward_layer(0, sX, a.pin / 16, sHL);
        }
        backward_layer(2, sD, a.pout / 16, sHL, wave < bands_out, dWo);
        if (two) {
            backward_layer(3, sHL, 8, sH1, true, dW2);
            first_layer(sH1);
        } else {
            first_layer(sHL);
        }
        __syncthreads();
        if (want_dx) mlp_store_tile<ML_BT, ML_BP>(sD, a.dx, p0, (size_t)a.N, a.n_in, tid);
        __syncthreads();
    }
    if (!want_dp) return;
    // ---- this workgroup's partial sums
    float* __restrict__ pw = a.partW + (size_t)blockIdx.x * 3 * ML_MAT;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int e = mlp_row(wave, bk, v) * ML_H + 32 * t + bn;
            pw[e] = dW1[t][v];
            if (two) pw[ML_MAT + e] = dW2[t][v];
            pw[2 * ML_MAT + e] = dWo[t][v];
        }
}

// partial sums of the G workgroups -> d_params in the flat layout.  One thread per element adds its partials in workgroup order;
// the loads of 16 partials are issued together (k_uv_backward_reduce)
__global__ void __launch_bounds__(256)
k_mlp_backward_reduce(const float* __restrict__ partW, int G, float* __restrict__ d_params, int pin, int pout, int L) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int n1 = ML_H * pin, n2 = (L - 1) * ML_MAT, n3 = pout * ML_H;
    if (e >= n1 + n2 + n3) return;
    int src;
    if (e < n1) { const int r = e / pin; src = r * ML_H + (e - r * pin); }
    else if (e < n1 + n2) src = ML_MAT + (e - n1);
    else src = 2 * ML_MAT + (e - n1 - n2);
    const float* __restrict__ p = partW + src;
    constexpr size_t stride = 3 * ML_MAT;
    float v = 0.0f;
    int g = 0;
    for (; g + 16 <= G; g += 16) {
        float t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = p[(size_t)(g + k) * stride];
#pragma unroll
        for (int k = 0; k < 16; ++k) v += t[k];
    }
    for (; g < G; ++g) v += p[(size_t)g * stride];
    d_params[e] = v;
}

int pad16(int k) { return (k + 15) / 16 * 16; }

}  // namespace

static size_t mlp_param_count(const TexGSMlp* m) {
    return (size_t)ML_H * pad16(m->n_in) + (size_t)(m->n_hidden_layers - 1) * ML_MAT + (size_t)pad16(m->n_out) * ML_H;
}

static size_t mlp_forward_temp_bytes() { return (size_t)ML_FWD_MATS * ML_MAT_BYTES; }

static int mlp_backward_blocks(int N) {
    const int t = (N + ML_BT - 1) / ML_BT;
    return t < TEXGS_MLP_BACKWARD_MAX_WORKGROUPS ? (t < 1 ? 1 : t) : TEXGS_MLP_BACKWARD_MAX_WORKGROUPS;
}

static size_t mlp_backward_temp_bytes(int N) {
    return (size_t)ML_BWD_MATS * ML_MAT_BYTES + (size_t)mlp_backward_blocks(N) * 3 * ML_MAT_BYTES;
}

// the matrices of `params` as pack records: W_1 [128, pin], W_2 [128, 128] (L = 2), W_out [pout, 128]
static void mlp_mats(const TexGSMlp* m, MlpPackMat& w1, MlpPackMat& w2, MlpPackMat& wo) {
    const int pin = pad16(m->n_in), pout = pad16(m->n_out);
    w1 = {0, ML_H, pin, 0};
    w2 = m->n_hidden_layers == 2 ? MlpPackMat{ML_H * pin, ML_H, ML_H, 0} : MlpPackMat{0, 0, 0, 0};
    wo = {ML_H * pin + (m->n_hidden_layers - 1) * ML_MAT, pout, ML_H, 0};
}

static hipError_t launch_mlp_forward(const TexGSMlp* m, const float* params, const float* x, int N, float* y, void* temp, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    MlpPackMat w1, w2, wo;
    mlp_mats(m, w1, w2, wo);
    const MlpPackArgs pa{{w1, w2, wo, {0, 0, 0, 0}, {0, 0, 0, 0}}};
    float* pk = reinterpret_cast<float*>(temp);
    hipLaunchKernelGGL(k_mlp_pack, dim3(ML_FWD_MATS * ML_MAT / 256), dim3(256), 0, s, params, pa, ML_FWD_MATS, pk);
    const MlpFwdArgs a{pk, x, y, N, m->n_in, m->n_out, pad16(m->n_in), pad16(m->n_out), m->n_hidden_layers};
    hipLaunchKernelGGL(k_mlp_forward, dim3((N + ML_FT - 1) / ML_FT), dim3(256), 0, s, a);
    return hipGetLastError();
}

static hipError_t launch_mlp_backward(const TexGSMlp* m, const float* params, const float* x, const float* dy, int N, float* dx, float* d_params,
                               void* temp, hipStream_t s) {
    LaunchStatus st;
    if (N <= 0) {                                          // no points: every gradient is zero
        if (d_params) st += hipMemsetAsync(d_params, 0, mlp_param_count(m) * sizeof(float), s);
        return st.first;
    }
    if (!dx && !d_params) return hipSuccess;
    MlpPackMat w1, w2, wo;
    mlp_mats(m, w1, w2, wo);
    auto T = [](MlpPackMat q) { q.trans = 1; return q; };
    const MlpPackArgs pa{{w1, w2, T(wo), T(w2), T(w1)}};
    float* pk = reinterpret_cast<float*>(temp);
    float* partW = pk + (size_t)ML_BWD_MATS * ML_MAT;
    const int G = mlp_backward_blocks(N);
    const int pin = pad16(m->n_in), pout = pad16(m->n_out), L = m->n_hidden_layers;
    hipLaunchKernelGGL(k_mlp_pack, dim3(ML_BWD_MATS * ML_MAT / 256), dim3(256), 0, s, params, pa, ML_BWD_MATS, pk);
    const MlpBwdArgs a{pk, x, dy, dx, d_params ? partW : nullptr, N, (N + ML_BT - 1) / ML_BT, m->n_in, m->n_out, pin, pout, L};
    hipLaunchKernelGGL(k_mlp_backward, dim3(G), dim3(256), 0, s, a);
    if (d_params) {
        const int n = (int)mlp_param_count(m);
        hipLaunchKernelGGL(k_mlp_backward_reduce, dim3((n + 255) / 256), dim3(256), 0, s, partW, G, d_params, pin, pout, L);
    }
    return st.after_launches();
}

extern "C" {

// include/texgs_mlp.h: the shape, by name
static int check_mlp(const TexGSMlp* m) {
    if (!m) return fail_msg("mlp is NULL");
    const char* what = nullptr;
    int v = 0;
    if (m->n_neurons != TEXGS_MLP_WIDTH) { what = "n_neurons must be 128"; v = m->n_neurons; }
    else if (m->n_hidden_layers < 1 || m->n_hidden_layers > TEXGS_MLP_MAX_HIDDEN_LAYERS) { what = "n_hidden_layers must be 1 or 2"; v = m->n_hidden_layers; }
    else if (m->n_in < 1 || m->n_in > TEXGS_MLP_WIDTH) { what = "n_in must be in [1,128]"; v = m->n_in; }
    else if (m->n_out < 1 || m->n_out > TEXGS_MLP_WIDTH) { what = "n_out must be in [1,128]"; v = m->n_out; }
    if (!what) return 0;
    return failf("the fused MLP does not support this shape: %s, got %d", what, v);
}

static int check_mlp_call(const TexGSMlp* m, int32_t N, const void* params, const void* temp) {
    if (int r = check_mlp(m)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (N > INT32_MAX - TEXGS_MLP_FORWARD_TILE) return fail_msg("N too large: the tile count is a 32-bit integer");
    if (!params || !temp) return fail_msg("NULL argument (params or temp)");
    if ((uintptr_t)params & 3) return fail_msg("params must be 4-byte aligned");
    if ((uintptr_t)temp & 15) return fail_msg("temp must be 16-byte aligned");
    return 0;
}

size_t texgs_mlp_param_count(const TexGSMlp* mlp) { return check_mlp(mlp) ? 0 : mlp_param_count(mlp); }

size_t texgs_mlp_forward_temp_bytes(const TexGSMlp* mlp, int32_t N) { return check_mlp(mlp) || N < 0 ? 0 : mlp_forward_temp_bytes(); }

size_t texgs_mlp_backward_temp_bytes(const TexGSMlp* mlp, int32_t N) { return check_mlp(mlp) || N < 0 ? 0 : mlp_backward_temp_bytes(N); }

int texgs_mlp_forward(const TexGSMlp* mlp, const float* params, const float* x, int32_t N, float* y, void* temp, void* stream) {
    if (int r = check_mlp_call(mlp, N, params, temp)) return r;
    if (N == 0) return 0;
    if (!x || !y) return fail_msg("NULL argument (x or y)");
    if (((uintptr_t)x | (uintptr_t)y) & 3) return fail_msg("x and y must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("mlp_forward", launch_mlp_forward(mlp, params, x, N, y, temp, s), s, false);
}

int texgs_mlp_backward(const TexGSMlp* mlp, const float* params, const float* x, const float* dy, int32_t N, float* dx, float* d_params,
                       void* temp, void* stream) {
    if (int r = check_mlp_call(mlp, N, params, temp)) return r;
    if (N > 0 && (!x || !dy)) return fail_msg("NULL argument (x or dy)");
    if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)d_params) & 3) return fail_msg("x, dy, dx and d_params must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("mlp_backward", launch_mlp_backward(mlp, params, x, dy, N, dx, d_params, temp, s), s, false);
}

}  // extern "C"
