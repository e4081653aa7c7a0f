/*
 * texgs_lpips_grad.h -- the backward of LPIPS-VGG in the images (csrc/lpips_grad.hip): the streaming kernels that stand between the
 * data-gradient convolutions.  The data gradient of a 3x3 / stride 1 / padding 1 convolution is texgs_conv3x3 (texgs_lpips.h) itself,
 * called with the weights transposed in the channel axes and flipped in both taps, relu = 0, pool_in = 0, no affine and a zero bias;
 * texgs/lpips.py chains thirteen of them with the two entry points below.  Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is
 * unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().  Every argument is checked before the first launch, so a
 * refused call has changed nothing.  No entry point waits on the host, reads anything back or allocates; no atomics: two calls give
 * the same bits.
 */
#ifndef TEXGS_LPIPS_GRAD_H
#define TEXGS_LPIPS_GRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_LPIPS_WRT_FIRST 1       /* bits of `wrt`: the first images (slots 0 .. P-1 of f) */
#define TEXGS_LPIPS_WRT_PARTNER 2     /* their partners (slots P .. 2P-1 of f) */

/* The backward of one tapped layer, ONE launch: the head's gradient in the tapped map, the max-pool's backward of the gradient that
 * arrives from the next slice, and the ReLU gate of the convolution that wrote the map.
 *
 * f f32[2P, C, h, w] is the tapped (post-ReLU) map as texgs_lpips_head takes it, gbar f32[P] the upstream gradient of each pair's
 * value.  Per pixel, in f32 with one rounding per operation and every sum in channel order (eps = 1e-10f):
 *     n0 = sqrt(sum_c f0_c^2),  d0 = n0 + eps,  n1, d1 likewise
 *     r_c = (2 lin_c) (f0_c / d0 - f1_c / d1)
 *     t0 = sum_c r_c f0_c,  t1 = sum_c r_c f1_c,  s = gbar_p / (float)(h w)
 *     head0_c = s (  r_c / d0 - f0_c (  t0 / (n0 (d0 d0))))
 *     head1_c = s ((-r_c) / d1 - f1_c ((-t1) / (n1 (d1 d1))))
 * head1 is head0 with the two images swapped, bit for bit.  A pixel whose n is 0 gets a zero row -- a deliberate deviation from the
 * derivative of sqrt at 0, which is not finite.
 *
 * G[c, y, x] = f[c, y, x] > 0 ? unpool(g_next)[c, y, x] + head[c, y, x] : 0.
 * g_next f32[B', C, h / 2, w / 2] (dense) is the data gradient that the next slice's first convolution produced, or NULL (layer 4):
 * unpool routes g_next[c, y', x'] to the FIRST maximum of f in the window rows 2y', 2y' + 1 x columns 2x', 2x' + 1, in row-major
 * order; pixels of an odd last row or column belong to no window and receive the head term only.
 *
 * G and g_next hold the B' images that `wrt` selects, in slot order: the P first images (wrt = 1), the P partners (wrt = 2), or all
 * 2P as in f (wrt = 3).  Nothing else is written.  G may be a view into a larger buffer: g_row, g_chan, g_img are the distances in
 * floats from a row, a channel plane and an image to the next (columns are adjacent); all three 0 means dense (w, h w, C h w),
 * otherwise row >= w, chan >= h x row, img >= C x chan.
 * Limits: 1 <= P <= 65535, 1 <= C <= 512, h, w >= 1, h w < 2^31, wrt in 1..3, h >= 2 and w >= 2 with g_next;
 * every pointer 4-byte aligned.  Anything else is refused by name. */
typedef struct TexGSLpipsHeadBackward {
    const float* f;
    const float* lin;            /* f32[C] */
    const float* gbar;           /* f32[P] */
    const float* g_next;         /* f32[B', C, h / 2, w / 2] or NULL */
    float* G;                    /* f32[B', C, h, w] */
    int32_t P, C, h, w;
    int32_t wrt;                 /* TEXGS_LPIPS_WRT_* bits */
    int64_t g_row, g_chan, g_img;        /* strides of G in floats; 0, 0, 0: dense */
} TexGSLpipsHeadBackward;

int texgs_lpips_head_backward(const TexGSLpipsHeadBackward* d, void* stream);

/* The ReLU gate between two data-gradient convolutions, in place: G[i] = y[i] > 0 ? G[i] : 0 for i < n, where y is the post-ReLU
 * output of the convolution whose input gradient G is (so -0 and 0 close the gate, and a closed gate stores +0 whatever G held).
 * Limits: 1 <= n < 2^40; G and y 16-byte aligned (16 bytes move per lane; the last n % 4 elements are handled one by one). */
int texgs_lpips_gate(float* G, const float* y, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_LPIPS_GRAD_H */
