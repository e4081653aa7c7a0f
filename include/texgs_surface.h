/*
 * texgs_surface.h -- the surface-point stage of libtexgs.so (csrc/surface.hip): what the reference's models do to a rendered depth
 * map before the UV networks see it (models/uv_map_gaussian3d.py:180-183, :271-286; models/texture_gaussian3d.py:394-400) --
 * unproject every pixel to a world point, keep the pixels whose alpha passes a threshold, in pixel order -- and the composite that
 * puts per-point colours back onto the pixel grid.  Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is unchanged); plain C99,
 * nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.  No atomics, no workgroup waits on another, no host wait, no readback: two calls give the same
 * bits.  P = height * width, 1 <= P < 2^31, each side at most TEXGS_SURFACE_MAX_SIDE.
 *
 * The arithmetic is a bit-exact contract (tests/surface_ref.py states it in numpy with the same operation order): every operation
 * rounded once, no fused multiply-add, IEEE division.
 */
#ifndef TEXGS_SURFACE_H
#define TEXGS_SURFACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_SURFACE_PIXELS_PER_THREAD 4           /* a thread takes 4 consecutive pixels (one 16-byte load per plane) */
#define TEXGS_SURFACE_PIXELS_PER_WORKGROUP 1024     /* 256 threads of 4 pixels: the pixels one per-workgroup count covers */
#define TEXGS_SURFACE_SCAN_WIDTH 256                /* counts the scanning workgroup takes per pass; more counts: it loops */
#define TEXGS_SURFACE_MAX_SIDE 16384

/* texgs_surface_points.  A pixel p = y * width + x is SELECTED when alpha[p] > threshold (strict: a NaN alpha is not selected).
 * The selected pixels are numbered r = 0, 1, ... in pixel order (a stable compaction); *count receives their number M.
 *
 * Once per call, in fp64 (B = the inverse of the float32 matrix full_proj, row-major a[4 i + j], as adjugate over determinant):
 *     s0 = a00 a11 - a10 a01   s1 = a00 a12 - a10 a02   s2 = a00 a13 - a10 a03
 *     s3 = a01 a12 - a11 a02   s4 = a01 a13 - a11 a03   s5 = a02 a13 - a12 a03
 *     c5 = a22 a33 - a32 a23   c4 = a21 a33 - a31 a23   c3 = a21 a32 - a31 a22
 *     c2 = a20 a33 - a30 a23   c1 = a20 a32 - a30 a22   c0 = a20 a31 - a30 a21
 *     det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0
 *     T(p, q, r; u, v, w) = ((p u) - (q v)) + (r w)
 *     B00 =  T(a11, a12, a13; c5, c4, c3) / det   B01 = -T(a01, a02, a03; c5, c4, c3) / det   B02 =  T(a31, a32, a33; s5, s4, s3) / det
 *     B10 = -T(a10, a12, a13; c5, c2, c1) / det   B11 =  T(a00, a02, a03; c5, c2, c1) / det   B12 = -T(a30, a32, a33; s5, s2, s1) / det
 *     B20 =  T(a10, a11, a13; c4, c2, c0) / det   B21 = -T(a00, a01, a03; c4, c2, c0) / det   B22 =  T(a30, a31, a33; s4, s2, s0) / det
 *     B30 = -T(a10, a11, a12; c3, c1, c0) / det   B31 =  T(a00, a01, a02; c3, c1, c0) / det   B32 = -T(a30, a31, a32; s3, s1, s0) / det
 * (the fourth column is not needed).  A singular matrix gives non-finite points; it is not checked (that would need a readback).
 *
 * Per selected pixel, in fp64, d = depth[p]:
 *     ndc_x = (2 x + 1) / width - 1          ndc_y = (2 y + 1) / height - 1
 *     z     = (zfar d) / (zfar - znear) - (zfar znear) / (zfar - znear)
 *     q     = (ndc_x d, ndc_y d, z, d)
 *     xyz[r][j] = (float) (((q0 B0j + q1 B1j) + q2 B2j) + q3 B3j)          j = 0, 1, 2: one rounding to float32
 * and index[r] = p, alpha_sel[r] = alpha[p]; rank[p] = r for a selected pixel and -1 otherwise.  Rows at and past M are not written.
 *
 * Three launches: per-workgroup counts (64-bit ballots, popcount) into temp; one workgroup scans the counts, writes *count and the
 * twelve B entries into temp; the third re-forms the ballots, ranks the lanes and writes the outputs.
 * depth, alpha, full_proj, xyz, alpha_sel, rank, count: 4-byte aligned (depth and alpha are read 16 bytes at a time when they are
 * 16-byte aligned); index and temp: 8-byte aligned. */
typedef struct TexGSSurfacePoints {
    const float* depth;         /* [H, W] */
    const float* alpha;         /* [H, W] */
    const float* full_proj;     /* 16 floats, row-major, the reference's row-vector convention: clip = [p, 1] @ P */
    float* xyz;                 /* [capacity, 3] */
    int64_t* index;             /* [capacity], or NULL */
    float* alpha_sel;           /* [capacity], or NULL */
    int32_t* rank;              /* [H * W], or NULL */
    uint32_t* count;            /* one word */
    double zfar;
    double znear;               /* zfar == znear is refused */
    float threshold;            /* a NaN is refused */
    int32_t height;
    int32_t width;
    int32_t capacity;           /* rows of xyz, index and alpha_sel: at least H * W (the count is not known before the launches) */
} TexGSSurfacePoints;

/* texgs_surface_compose: the composite of uv_map_gaussian3d.py:283-286 without scatter_add, per pixel p and channel c, in fp32:
 *     r = rank[p];  sel = 0 <= r < rows
 *     out[c * P + p] = (bg[c] * (1.0f - alpha[p])) + (sel ? alpha[p] * values[3 r + c] : 0.0f)
 * background NULL is 0, 0, 0.  rows == 0 (values may then be NULL) writes the background term everywhere.  A rank outside [0, rows)
 * counts as unselected, so `values` is never read out of bounds.  All pointers 4-byte aligned. */
typedef struct TexGSSurfaceCompose {
    const float* values;        /* [rows, 3] */
    const int32_t* rank;        /* [H, W], as texgs_surface_points leaves it */
    const float* alpha;         /* [H, W] */
    const float* background;    /* 3 floats on the device, or NULL */
    float* out;                 /* [3, H, W] */
    int32_t rows;
    int32_t height;
    int32_t width;
} TexGSSurfaceCompose;

/* Bytes of `temp` (8-byte aligned) for texgs_surface_points; 0 for an image it refuses.  The next call on the same stream may reuse it. */
size_t texgs_surface_temp_bytes(int32_t height, int32_t width);

int texgs_surface_points(const TexGSSurfacePoints* s, void* temp, size_t temp_bytes, void* stream);
int texgs_surface_compose(const TexGSSurfaceCompose* c, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_SURFACE_H */
