// The input stage (include/texgs_ingest.h): a view's 8-bit files as the tensors the losses read, from the uploaded bytes.
//   k_taps       one axis of Pillow's tap tables, a thread per output index, in fp64 (precompute_coeffs + normalize_coeffs_8bpc)
//   k_hpass      the horizontal pass: lanes along output x, the rows' input span staged in LDS as whole dwords
//   k_vpass      the vertical pass: a thread per quad of 4 output pixels, dword loads of the rows above and below
//   k_decode     the decode alone, when neither size changes
//   k_composite  dataset_readers.py:219-225: RGBA over a background, fp64
// The decode (utils/general.py:23, cameras.py:49,117,122) is fused into whichever pass is the last.
// Everything here is a bit-exact contract (tests/ingest_ref.py): the unit is built with -ffp-contract=off, every fp64 / fp32
// operation below is rounded once, the divisions are IEEE, the sums are int32.
//
// Bytes.  Rows of the source and of out_u8 are W*C bytes with no alignment, so no kernel loads or stores a byte where a dword will
// do: global memory is read as aligned dwords and the wanted bytes are shifted out of a pair of them (`window`); k_hpass reads its
// bytes from LDS; 8-bit results leave as whole aligned dwords except at the 1..3 bytes where a span begins or ends off a dword.
// Only the LAST dword of a caller's buffer is read bytewise when the buffer ends inside it (`ld_dword`), so nothing is read past an
// end.  The intermediate between the passes lives in `temp` with its rows padded to whole dwords and indexed by SOURCE row.
#include "common.h"
#include "abi_support.h"
#include "texgs_ingest.h"

#include <math.h>

namespace {

constexpr int IB = 256;                     // threads of every workgroup here
constexpr int H_ROWS = IB / 64;             // k_hpass: a wave per source row
constexpr uint32_t H_CAP = 8192;            // k_hpass: LDS bytes that stage one row's input span (2730 rgb pixels)
constexpr int H_TX = 64;                    // k_hpass: at most a wave of output pixels per tile
constexpr int32_t ROUND = 1 << (TEXGS_INGEST_PRECISION_BITS - 1);
constexpr int MAX_GRID = 4096;              // of the grid-stride kernels

__host__ __device__ inline double filter_support(int filter) {
    return filter == TEXGS_INGEST_BICUBIC ? 2.0 : (filter == TEXGS_INGEST_BILINEAR ? 1.0 : 0.5);
}

// Pillow's filters (Resample.c), operation for operation
__device__ __forceinline__ double filter_value(int filter, double x) {
    if (filter == TEXGS_INGEST_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    if (x < 0.0) x = -x;
    if (filter == TEXGS_INGEST_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

struct Axis {           // what every output index of one axis shares
    double scale, support, ss;
    int ksize;
};

__host__ __device__ inline Axis make_axis(int inS, int outS, int filter) {
    Axis a;
    a.scale = (double)inS / (double)outS;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = filter_support(filter) * fs;
    a.ss = 1.0 / fs;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}

// (xmin, n) of output index xx: the same code on the host (the rows the horizontal pass runs over) and in k_taps
__host__ __device__ inline void axis_bounds(const Axis& a, int inS, int xx, double& center, int& xmin, int& n) {
    center = (xx + 0.5) * a.scale;
    xmin = (int)(center - a.support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + a.support + 0.5);
    if (xmax > inS) xmax = inS;
    n = xmax - xmin;
    if (n > a.ksize) n = a.ksize;       // (never: Pillow sizes its rows by ksize as well)
}

__global__ void __launch_bounds__(IB)
k_taps(int inS, int outS, int filter, int32_t* __restrict__ taps /* [ksize][outS] */, int32_t* __restrict__ bounds /* [outS][2] */) {
    const int xx = blockIdx.x * IB + threadIdx.x;
    if (xx >= outS) return;
    const Axis a = make_axis(inS, outS, filter);
    double center;
    int xmin, n;
    axis_bounds(a, inS, xx, center, xmin, n);
    double ww = 0.0;            // the weights are evaluated twice rather than kept: the same operations give the same values
    for (int x = 0; x < n; ++x) ww += filter_value(filter, (x + xmin - center + 0.5) * a.ss);
    for (int x = 0; x < n; ++x) {
        double p = filter_value(filter, (x + xmin - center + 0.5) * a.ss);
        if (ww != 0.0) p /= ww;
        taps[(size_t)x * outS + xx] = p < 0 ? (int)(p * 4194304.0 - 0.5) : (int)(p * 4194304.0 + 0.5);
    }
    for (int x = n; x < a.ksize; ++x) taps[(size_t)x * outS + xx] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
}

// ---- bytes through dwords ----
// The aligned dword at byte a0 of a buffer of `size` bytes; the buffer's last dword is read bytewise when the buffer ends inside it
__device__ __forceinline__ uint32_t ld_dword(const uint8_t* __restrict__ base, uint32_t a0, uint32_t size) {
    if (a0 + 4u <= size) return *reinterpret_cast<const uint32_t*>(base + a0);
    uint32_t v = 0;
    for (uint32_t b = 0; b < 3u; ++b)
        if (a0 + b < size) v |= (uint32_t)base[a0 + b] << (8u * b);
    return v;
}

// The 4 bytes that start `sh` bytes into the dword pair (lo, hi)
__device__ __forceinline__ uint32_t window(uint32_t lo, uint32_t hi, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh));
}

__device__ __forceinline__ uint32_t clip8(int32_t acc) {
    const int32_t v = acc >> TEXGS_INGEST_PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- the decode ----
struct Decode {
    const float* mul;       // [P] or NULL
    uint8_t* u8;            // [P, C] or NULL
    float* chw;             // [C, P] or NULL
    float* mask;            // [P] or NULL
    uint32_t P;
    int C;
    int is_signed;
    int wide;               // chw, mask and mul take 16-byte accesses at a quad (the host checked pointers and P)
};

__device__ __forceinline__ float decode_value(uint32_t b, bool is_signed) {
    float v = (float)b / 255.0f;
    if (is_signed) v = (v * 2.0f) - 1.0f;
    return v;
}

// One quad's outputs: b[k][c] are the bytes of pixel p0 + k; n <= 4 of them exist
__device__ __forceinline__ void emit_quad(const Decode& d, uint32_t p0, uint32_t n, const uint32_t (&b)[4][3]) {
    if (d.u8) {
        if (n == 4u) {
            if (d.C == 3) {
                uint32_t* o = reinterpret_cast<uint32_t*>(d.u8 + (size_t)p0 * 3);
                o[0] = b[0][0] | (b[0][1] << 8) | (b[0][2] << 16) | (b[1][0] << 24);
                o[1] = b[1][1] | (b[1][2] << 8) | (b[2][0] << 16) | (b[2][1] << 24);
                o[2] = b[2][2] | (b[3][0] << 8) | (b[3][1] << 16) | (b[3][2] << 24);
            } else {
                *reinterpret_cast<uint32_t*>(d.u8 + p0) = b[0][0] | (b[1][0] << 8) | (b[2][0] << 16) | (b[3][0] << 24);
            }
        } else {        // the image's last 1..3 pixels: bytes
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k)
                if (k < n)
                    for (int c = 0; c < d.C; ++c) d.u8[(size_t)(p0 + k) * d.C + c] = (uint8_t)b[k][c];
        }
    }
    const bool wide = d.wide && n == 4u;
    float m[4] = {1.f, 1.f, 1.f, 1.f};
    if (d.chw && d.mul) {
        if (wide) {
            const float4 t = *reinterpret_cast<const float4*>(d.mul + p0);
            m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (k < n) m[k] = d.mul[p0 + k];
        }
    }
    if (d.chw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < d.C) {
                float v[4];
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    v[k] = decode_value(b[k][c], d.is_signed);
                    if (d.mul) v[k] = v[k] * m[k];
                }
                float* o = d.chw + (size_t)c * d.P + p0;
                if (wide) {
                    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k)
                        if (k < n) o[k] = v[k];
                }
            }
        }
    }
    if (d.mask) {
        float* o = d.mask + p0;
        if (wide) {
            *reinterpret_cast<float4*>(o) = make_float4(b[0][0] ? 1.f : 0.f, b[1][0] ? 1.f : 0.f, b[2][0] ? 1.f : 0.f, b[3][0] ? 1.f : 0.f);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (k < n) o[k] = b[k][0] ? 1.f : 0.f;
        }
    }
}

// ---- the horizontal pass ----
struct HArgs {
    const uint8_t* src;         // [H, inW, C]
    const int32_t* taps;        // [ksize][outW]
    const int32_t* bounds;      // [outW][2]
    uint8_t* dst;               // rows of dst_pitch bytes, indexed by the SOURCE row; NULL when only floats are asked for
    Decode dec;                 // the float outputs, when this pass is the last (dec.u8 is not used: dst is)
    uint32_t src_size;          // bytes of src
    uint32_t dst_pitch;
    int inW, outW, C;
    int row0, rows;             // the source rows to run over
    int tx;                     // output pixels per tile: a multiple of 4, at most H_TX, chosen so that a tile's span fits H_CAP
    int last;                   // this pass is the last: write dec's floats
    uint32_t cap;               // LDS bytes that stage one row's span: what a tile of tx outputs can need, a multiple of 4, <= H_CAP
};

// blockIdx.x: the tile of tx output pixels; blockIdx.y: a group of H_ROWS rows, one per wave.
// Dynamic LDS: H_ROWS staging rows of a.cap bytes (a 2 x reduction needs 0.4 KiB a row, not H_CAP: twice the waves fit a CU).
__global__ void __launch_bounds__(IB)
k_hpass(HArgs a) {
    extern __shared__ uint32_t s_stage[];
    __shared__ uint32_t s_out[H_ROWS][H_TX * 3 / 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = a.row0 + blockIdx.y * H_ROWS + wave;
    const bool active = r < a.row0 + a.rows;
    const int x0 = blockIdx.x * a.tx, nx = min(a.tx, a.outW - x0), xl = x0 + nx - 1;
    const int C = a.C;
    // the tile's input span [start, end) of this wave's row, staged as the aligned dwords that hold it
    const int start = a.bounds[2 * x0], end = a.bounds[2 * xl] + a.bounds[2 * xl + 1];
    const uint32_t g = (uint32_t)r * (uint32_t)(a.inW * C) + (uint32_t)(start * C), g0 = g & ~3u, sh = g & 3u;
    const int xx = x0 + (lane < nx ? lane : 0);         // this lane's output, its bounds asked for before the staging loads
    const int xmin = a.bounds[2 * xx];
    int n = a.bounds[2 * xx + 1];
    uint32_t* s_in = s_stage + (size_t)wave * (a.cap / 4u);
    if (active) {
        uint32_t ndw = ((uint32_t)((end - start) * C) + sh + 3u) / 4u;
        if (ndw > a.cap / 4u) ndw = a.cap / 4u;     // (never: the host chose tx and cap for it)
        for (uint32_t i = lane; i < ndw; i += 64) s_in[i] = ld_dword(a.src, g0 + 4u * i, a.src_size);
    }
    __syncthreads();
    const uint8_t* in = reinterpret_cast<const uint8_t*>(s_in);
    uint8_t* ob = reinterpret_cast<uint8_t*>(s_out[wave]);
    if (active && lane < nx) {
        const uint32_t base = sh + (uint32_t)((xmin - start) * C);
        if (base + (uint32_t)(n * C) > a.cap) n = 0;        // (never)
        int32_t acc[3] = {ROUND, ROUND, ROUND};
        // four taps at a time, so that their (coalesced, but dependent on nothing) global loads are in flight together
        for (int k0 = 0; k0 < n; k0 += 4) {
            int32_t t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = k0 + j < n ? a.taps[(size_t)(k0 + j) * a.outW + xx] : 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (k0 + j < n) {
                    if (C == 3) {
                        const uint8_t* px = in + base + 3 * (k0 + j);
                        acc[0] += t[j] * (int32_t)px[0]; acc[1] += t[j] * (int32_t)px[1]; acc[2] += t[j] * (int32_t)px[2];
                    } else {
                        acc[0] += t[j] * (int32_t)in[base + k0 + j];
                    }
                }
            }
        }
        uint32_t b[3];
        for (int c = 0; c < C; ++c) { b[c] = clip8(acc[c]); ob[lane * C + c] = (uint8_t)b[c]; }
        if (a.last) {       // lanes run along x: every plane's stores are contiguous
            const Decode& d = a.dec;
            const uint32_t p = (uint32_t)r * (uint32_t)a.outW + (uint32_t)xx;
            if (d.chw) {
                const float m = d.mul ? d.mul[p] : 1.f;
                for (int c = 0; c < C; ++c) {
                    float v = decode_value(b[c], d.is_signed);
                    if (d.mul) v = v * m;
                    d.chw[(size_t)c * d.P + p] = v;
                }
            }
            if (d.mask) d.mask[p] = b[0] ? 1.f : 0.f;
        }
    }
    __syncthreads();
    if (active && a.dst) {      // the tile's nx * C bytes to dst at byte o, as aligned dwords; bytes only where it begins or ends off one
        const uint32_t o = (uint32_t)r * a.dst_pitch + (uint32_t)(x0 * C), L = (uint32_t)(nx * C);
        const uint32_t A = (o & ~3u) + 4u * lane;       // (L <= 192: one dword per lane is enough)
        if (A < o + L) {
            if (A >= o && A + 4u <= o + L) {
                const uint8_t* s = ob + (A - o);
                *reinterpret_cast<uint32_t*>(a.dst + A) = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
            } else {
                for (uint32_t k = 0; k < 4u; ++k)
                    if (A + k >= o && A + k < o + L) a.dst[A + k] = ob[A + k - o];
            }
        }
    }
}

// ---- the vertical pass ----
struct VArgs {
    const uint8_t* src;         // rows of src_pitch bytes, indexed by the source row: the intermediate, or the source itself
    const int32_t* taps;        // [ksize][outH]
    const int32_t* bounds;      // [outH][2]
    Decode dec;
    uint32_t src_size, src_pitch;
    int W, outH;
};

// A thread per quad of 4 output pixels, numbered flat over the image (4 pixels are whole dwords of every output).  A quad inside
// one row shares its taps and reads each source row as 3 or 4 aligned dwords (2 with one channel); a quad across a row's end, or
// the image's last, partial one, goes pixel by pixel.
__global__ void __launch_bounds__(IB)
k_vpass(VArgs a) {
    const Decode& d = a.dec;
    const uint32_t P = d.P, nq = (P + 3u) / 4u, W = (uint32_t)a.W;
    const int C = d.C;
    for (uint32_t q = blockIdx.x * IB + threadIdx.x; q < nq; q += gridDim.x * IB) {
        const uint32_t p0 = q * 4u, n = P - p0 < 4u ? P - p0 : 4u;
        const uint32_t y0 = p0 / W, x0 = p0 - y0 * W;
        int32_t acc[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = ROUND;
        if (n == 4u && x0 + 4u <= W) {
            const int ymin = a.bounds[2 * y0], nk = a.bounds[2 * y0 + 1];
            for (int k = 0; k < nk; ++k) {
                const int32_t t = a.taps[(size_t)k * a.outH + y0];
                const uint32_t off = (uint32_t)(ymin + k) * a.src_pitch + x0 * (uint32_t)C, a0 = off & ~3u, sh = off & 3u;
                const uint32_t d0 = ld_dword(a.src, a0, a.src_size);
                if (C == 3) {
                    const uint32_t d1 = ld_dword(a.src, a0 + 4u, a.src_size), d2 = ld_dword(a.src, a0 + 8u, a.src_size);
                    const uint32_t d3 = sh ? ld_dword(a.src, a0 + 12u, a.src_size) : 0u;
                    const uint32_t w0 = window(d0, d1, sh), w1 = window(d1, d2, sh), w2 = window(d2, d3, sh);
                    acc[0][0] += t * (int32_t)(w0 & 255u); acc[0][1] += t * (int32_t)((w0 >> 8) & 255u); acc[0][2] += t * (int32_t)((w0 >> 16) & 255u);
                    acc[1][0] += t * (int32_t)(w0 >> 24); acc[1][1] += t * (int32_t)(w1 & 255u); acc[1][2] += t * (int32_t)((w1 >> 8) & 255u);
                    acc[2][0] += t * (int32_t)((w1 >> 16) & 255u); acc[2][1] += t * (int32_t)(w1 >> 24); acc[2][2] += t * (int32_t)(w2 & 255u);
                    acc[3][0] += t * (int32_t)((w2 >> 8) & 255u); acc[3][1] += t * (int32_t)((w2 >> 16) & 255u); acc[3][2] += t * (int32_t)(w2 >> 24);
                } else {
                    const uint32_t d1 = sh ? ld_dword(a.src, a0 + 4u, a.src_size) : 0u;
                    const uint32_t w0 = window(d0, d1, sh);
                    acc[0][0] += t * (int32_t)(w0 & 255u); acc[1][0] += t * (int32_t)((w0 >> 8) & 255u);
                    acc[2][0] += t * (int32_t)((w0 >> 16) & 255u); acc[3][0] += t * (int32_t)(w0 >> 24);
                }
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                if (i < n) {
                    const uint32_t p = p0 + i, y = p / W, x = p - y * W;
                    const int ymin = a.bounds[2 * y], nk = a.bounds[2 * y + 1];
                    for (int k = 0; k < nk; ++k) {
                        const int32_t t = a.taps[(size_t)k * a.outH + y];
                        const uint32_t off = (uint32_t)(ymin + k) * a.src_pitch + x * (uint32_t)C, a0 = off & ~3u, sh = off & 3u;
                        const uint32_t lo = ld_dword(a.src, a0, a.src_size);
                        const uint32_t hi = sh + (uint32_t)C > 4u ? ld_dword(a.src, a0 + 4u, a.src_size) : 0u;
                        const uint32_t w0 = window(lo, hi, sh);
                        acc[i][0] += t * (int32_t)(w0 & 255u); acc[i][1] += t * (int32_t)((w0 >> 8) & 255u); acc[i][2] += t * (int32_t)((w0 >> 16) & 255u);
                    }
                }
            }
        }
        uint32_t b[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) { b[k][0] = clip8(acc[k][0]); b[k][1] = clip8(acc[k][1]); b[k][2] = clip8(acc[k][2]); }
        emit_quad(d, p0, n, b);
    }
}

// ---- the decode alone ----
__global__ void __launch_bounds__(IB)
k_decode(const uint8_t* __restrict__ src, uint32_t src_size, Decode d) {
    const uint32_t P = d.P, nq = (P + 3u) / 4u;
    for (uint32_t q = blockIdx.x * IB + threadIdx.x; q < nq; q += gridDim.x * IB) {
        const uint32_t p0 = q * 4u, n = P - p0 < 4u ? P - p0 : 4u;
        uint32_t b[4][3];
        if (d.C == 3) {        // 4 pixels are 3 aligned dwords
            const uint32_t w0 = ld_dword(src, p0 * 3u, src_size);
            const uint32_t w1 = n > 1u ? ld_dword(src, p0 * 3u + 4u, src_size) : 0u, w2 = n > 2u ? ld_dword(src, p0 * 3u + 8u, src_size) : 0u;
            b[0][0] = w0 & 255u; b[0][1] = (w0 >> 8) & 255u; b[0][2] = (w0 >> 16) & 255u;
            b[1][0] = w0 >> 24; b[1][1] = w1 & 255u; b[1][2] = (w1 >> 8) & 255u;
            b[2][0] = (w1 >> 16) & 255u; b[2][1] = w1 >> 24; b[2][2] = w2 & 255u;
            b[3][0] = (w2 >> 8) & 255u; b[3][1] = (w2 >> 16) & 255u; b[3][2] = w2 >> 24;
        } else {
            const uint32_t w0 = ld_dword(src, p0, src_size);
#pragma unroll
            for (int k = 0; k < 4; ++k) { b[k][0] = (w0 >> (8 * k)) & 255u; b[k][1] = b[k][2] = 0u; }
        }
        emit_quad(d, p0, n, b);
    }
}

// ---- the Blender loader's composite ----
__device__ __forceinline__ uint32_t composite_byte(uint32_t c, double na, double bg) {
    const double arr = (((double)c / 255.0) * na) + (bg * (1.0 - na));
    const double t = arr * 255.0;
    return t > 0.0 ? (t < 256.0 ? (uint32_t)(int)t : 255u) : 0u;
}

__global__ void __launch_bounds__(IB)
k_composite(const uint32_t* __restrict__ rgba, uint8_t* __restrict__ out, uint32_t P, double bg0, double bg1, double bg2) {
    const uint32_t nq = (P + 3u) / 4u;
    for (uint32_t q = blockIdx.x * IB + threadIdx.x; q < nq; q += gridDim.x * IB) {
        const uint32_t p0 = q * 4u, n = P - p0 < 4u ? P - p0 : 4u;
        uint32_t b[4][3];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t px = k < n ? rgba[p0 + k] : 0u;
            const double na = (double)(px >> 24) / 255.0;
            b[k][0] = composite_byte(px & 255u, na, bg0);
            b[k][1] = composite_byte((px >> 8) & 255u, na, bg1);
            b[k][2] = composite_byte((px >> 16) & 255u, na, bg2);
        }
        if (n == 4u) {
            uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)p0 * 3);
            o[0] = b[0][0] | (b[0][1] << 8) | (b[0][2] << 16) | (b[1][0] << 24);
            o[1] = b[1][1] | (b[1][2] << 8) | (b[2][0] << 16) | (b[2][1] << 24);
            o[2] = b[2][2] | (b[3][0] << 8) | (b[3][1] << 16) | (b[3][2] << 24);
        } else {
            for (uint32_t k = 0; k < n; ++k)
                for (int c = 0; c < 3; ++c) out[(size_t)(p0 + k) * 3 + c] = (uint8_t)b[k][c];
        }
    }
}

int quad_grid(uint32_t P) {
    const uint32_t g = ((P + 3u) / 4u + IB - 1) / IB;
    return (int)(g < (uint32_t)MAX_GRID ? g : (uint32_t)MAX_GRID);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

struct Plan {           // where everything lives in temp (byte offsets, all multiples of 4)
    int kh, kv;         // 0: that pass is skipped
    size_t taps_h, bounds_h, taps_v, bounds_v, inter, total;
    uint32_t pitch;     // of the intermediate
};

Plan make_plan(int H, int W, int C, int h, int w, int filter) {
    Plan p = {};
    size_t at = 0;
    if (w != W) {
        p.kh = make_axis(W, w, filter).ksize;
        p.taps_h = at; at += (size_t)p.kh * w * 4;
        p.bounds_h = at; at += (size_t)w * 8;
    }
    if (h != H) {
        p.kv = make_axis(H, h, filter).ksize;
        p.taps_v = at; at += (size_t)p.kv * h * 4;
        p.bounds_v = at; at += (size_t)h * 8;
    }
    p.pitch = (uint32_t)round4((size_t)w * C);
    if (p.kh && p.kv) { p.inter = at; at += (size_t)H * p.pitch; }
    p.total = at ? at : 4;
    return p;
}

}  // namespace

// (the arguments of these are validated by the entry points below)
static int ingest_ksize(int inS, int outS, int filter) { return make_axis(inS, outS, filter).ksize; }

static hipError_t launch_resize_taps(int inS, int outS, int filter, int32_t* taps, int32_t* bounds, hipStream_t s) {
    hipLaunchKernelGGL(k_taps, dim3((outS + IB - 1) / IB), dim3(IB), 0, s, inS, outS, filter, taps, bounds);
    return hipGetLastError();
}

static size_t resize_temp_bytes(int H, int W, int C, int h, int w, int filter) { return make_plan(H, W, C, h, w, filter).total; }

static hipError_t launch_resize_u8(const TexGSResize* r, void* temp, hipStream_t s) {
    const int H = r->src_height, W = r->src_width, C = r->channels, h = r->height, w = r->width;
    const Plan p = make_plan(H, W, C, h, w, r->filter);
    uint8_t* t = (uint8_t*)temp;
    const uint32_t P = (uint32_t)h * (uint32_t)w, src_size = (uint32_t)H * (uint32_t)W * (uint32_t)C;
    Decode d;
    d.mul = r->mul; d.u8 = r->out_u8; d.chw = r->out_chw; d.mask = r->out_mask; d.P = P; d.C = C;
    d.is_signed = (r->flags & TEXGS_INGEST_SIGNED) ? 1 : 0;
    d.wide = P % 4 == 0 && aligned16(r->out_chw) && aligned16(r->out_mask) && aligned16(r->mul);
    if (!p.kh && !p.kv) {
        hipLaunchKernelGGL(k_decode, dim3(quad_grid(P)), dim3(IB), 0, s, r->src, src_size, d);
        return hipGetLastError();
    }
    int row0 = 0, rows = H;
    if (p.kv) {
        int32_t* taps = (int32_t*)(t + p.taps_v);
        int32_t* bounds = (int32_t*)(t + p.bounds_v);
        hipLaunchKernelGGL(k_taps, dim3((h + IB - 1) / IB), dim3(IB), 0, s, H, h, r->filter, taps, bounds);
        if (p.kh) {     // the source rows the vertical pass reads: those of its first output row up to those of its last
            const Axis a = make_axis(H, h, r->filter);
            double center;
            int first, n0, last, n1;
            axis_bounds(a, H, 0, center, first, n0);
            axis_bounds(a, H, h - 1, center, last, n1);
            row0 = first;
            rows = last + n1 - first;
        }
    }
    if (p.kh) {
        const Axis a = make_axis(W, w, r->filter);
        HArgs ha;
        ha.src = r->src;
        ha.taps = (const int32_t*)(t + p.taps_h);
        ha.bounds = (const int32_t*)(t + p.bounds_h);
        ha.dec = d;
        ha.src_size = src_size;
        ha.inW = W; ha.outW = w; ha.C = C; ha.row0 = row0; ha.rows = rows;
        ha.last = p.kv ? 0 : 1;
        ha.dst = p.kv ? t + p.inter : r->out_u8;
        ha.dst_pitch = p.kv ? p.pitch : (uint32_t)(w * C);
        // a tile of tx outputs spans at most (tx - 1) * scale + ksize + 1 source pixels, and starts up to 3 bytes into its first dword
        const double cap_px = (double)((H_CAP - 4) / C);
        double fit = floor((cap_px - a.ksize - 2) / a.scale) + 1.0;
        ha.tx = fit >= (double)H_TX ? H_TX : ((int)fit & ~3);
        const double need = (ceil((ha.tx - 1) * a.scale) + a.ksize + 2) * C + 4;        // bytes, by the same bound
        ha.cap = need >= (double)H_CAP ? H_CAP : (uint32_t)round4((size_t)need);
        hipLaunchKernelGGL(k_taps, dim3((w + IB - 1) / IB), dim3(IB), 0, s, W, w, r->filter, (int32_t*)(t + p.taps_h), (int32_t*)(t + p.bounds_h));
        if (rows > 0)
            hipLaunchKernelGGL(k_hpass, dim3((w + ha.tx - 1) / ha.tx, (rows + H_ROWS - 1) / H_ROWS), dim3(IB), (size_t)H_ROWS * ha.cap, s, ha);
    }
    if (p.kv) {
        VArgs va;
        va.src = p.kh ? t + p.inter : r->src;
        va.taps = (const int32_t*)(t + p.taps_v);
        va.bounds = (const int32_t*)(t + p.bounds_v);
        va.dec = d;
        va.src_pitch = p.kh ? p.pitch : (uint32_t)(W * C);
        va.src_size = p.kh ? (uint32_t)H * p.pitch : src_size;
        va.W = w; va.outH = h;
        hipLaunchKernelGGL(k_vpass, dim3(quad_grid(P)), dim3(IB), 0, s, va);
    }
    return hipGetLastError();
}

static hipError_t launch_rgba_composite(const uint8_t* rgba, uint8_t* out, int H, int W, double bg0, double bg1, double bg2, hipStream_t s) {
    const uint32_t P = (uint32_t)H * (uint32_t)W;
    hipLaunchKernelGGL(k_composite, dim3(quad_grid(P)), dim3(IB), 0, s, (const uint32_t*)rgba, out, P, bg0, bg1, bg2);
    return hipGetLastError();
}

extern "C" {

// include/texgs_ingest.h: every argument is checked before the first launch, so a refused call has changed nothing
// One axis in_size -> out_size: its ksize, or 0 with the cause in the error text
static int check_resize_axis(const char* what, int32_t in_size, int32_t out_size, int32_t filter) {
    if (filter != TEXGS_INGEST_BICUBIC && filter != TEXGS_INGEST_BILINEAR && filter != TEXGS_INGEST_BOX) {
        failf("unknown filter %lld (TEXGS_INGEST_BICUBIC, _BILINEAR or _BOX)", (long long)filter);
        return 0;
    }
    if (in_size < 1 || out_size < 1) {
        failf("%s: sizes must be positive, got %d -> %d", what, in_size, out_size);
        return 0;
    }
    if (in_size > TEXGS_INGEST_MAX_SIDE || out_size > TEXGS_INGEST_MAX_SIDE) {
        failf("%s: %d -> %d: an image side above %d is not supported", what, in_size, out_size, TEXGS_INGEST_MAX_SIDE);
        return 0;
    }
    const int k = ingest_ksize(in_size, out_size, filter);
    if (k > TEXGS_INGEST_MAX_KSIZE) {
        failf("%s: %d -> %d needs ksize %d taps per output, above the limit of %d", what, in_size, out_size, k,
              TEXGS_INGEST_MAX_KSIZE);
        return 0;
    }
    return k;
}

static int check_resize_shape(int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, int32_t filter) {
    if (C == 4) return fail_msg("channels = 4 (RGBA) is not supported: Pillow premultiplies alpha before it resamples; composite first");
    if (C != 1 && C != 3) return failf("channels must be 1 or 3, got %lld", (long long)C);
    if (!check_resize_axis("width", W, w, filter) || !check_resize_axis("height", H, h, filter)) return -1;
    return 0;
}

int32_t texgs_resize_ksize(int32_t in_size, int32_t out_size, int32_t filter) { return check_resize_axis("axis", in_size, out_size, filter); }

int texgs_resize_taps(int32_t in_size, int32_t out_size, int32_t filter, int32_t* taps, int32_t* bounds, void* stream) {
    if (!check_resize_axis("axis", in_size, out_size, filter)) return -1;
    if (!taps || !bounds) return fail_msg("NULL argument (taps or bounds)");
    if (((uintptr_t)taps | (uintptr_t)bounds) & 3) return fail_msg("taps and bounds must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("resize_taps", launch_resize_taps(in_size, out_size, filter, taps, bounds, s), s, false);
}

size_t texgs_resize_temp_bytes(int32_t src_height, int32_t src_width, int32_t channels, int32_t height, int32_t width, int32_t filter) {
    return check_resize_shape(src_height, src_width, channels, height, width, filter)
               ? 0 : resize_temp_bytes(src_height, src_width, channels, height, width, filter);
}

int texgs_resize_u8(const TexGSResize* r, void* temp, size_t temp_bytes, void* stream) {
    if (!r) return fail_msg("resize descriptor is NULL");
    if (int e = check_resize_shape(r->src_height, r->src_width, r->channels, r->height, r->width, r->filter)) return e;
    if (!r->src || !temp) return fail_msg("NULL argument (src or temp)");
    if (r->flags & ~TEXGS_INGEST_SIGNED) return fail_msg("unknown bit in flags");
    if (!r->out_u8 && !r->out_chw && !r->out_mask) return fail_msg("no output requested (out_u8, out_chw and out_mask are all NULL)");
    if (r->mul && !r->out_chw) return fail_msg("mul is read with out_chw only");
    if (((uintptr_t)r->src | (uintptr_t)r->mul | (uintptr_t)r->out_u8 | (uintptr_t)r->out_chw | (uintptr_t)r->out_mask | (uintptr_t)temp) & 3)
        return fail_msg("src, mul, out_u8, out_chw, out_mask and temp must be 4-byte aligned");
    if (temp_bytes < resize_temp_bytes(r->src_height, r->src_width, r->channels, r->height, r->width, r->filter))
        return fail_msg("temp is smaller than texgs_resize_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("resize_u8", launch_resize_u8(r, temp, s), s, false);
}

int texgs_rgba_composite(const uint8_t* rgba, uint8_t* out, int32_t height, int32_t width, double bg_r, double bg_g, double bg_b,
                         void* stream) {
    if (height < 1 || width < 1) return fail_msg("height and width must be positive");
    if (height > TEXGS_INGEST_MAX_SIDE || width > TEXGS_INGEST_MAX_SIDE)
        return failf("%lld x %lld: an image side above 16384 is not supported", (long long)height, (long long)width);
    if (!rgba || !out) return fail_msg("NULL argument (rgba or out)");
    if (((uintptr_t)rgba | (uintptr_t)out) & 3) return fail_msg("rgba and out must be 4-byte aligned");
    if (!(bg_r >= 0.0 && bg_r <= 1.0 && bg_g >= 0.0 && bg_g <= 1.0 && bg_b >= 0.0 && bg_b <= 1.0))
        return fail_msg("the background must lie in [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    return launched("rgba_composite", launch_rgba_composite(rgba, out, height, width, bg_r, bg_g, bg_b, s), s, false);
}

}  // extern "C"
