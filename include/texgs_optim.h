/*
 * texgs_optim.h -- the optimizer entry point of libtexgs.so (csrc/optim.hip): one fused multi-tensor Adam step, what
 * models/texture_gaussian3d.py:420-444 of the reference spends in three torch.optim.Adam(..., eps=1e-15).step() calls and a zero_grad.
 * Additive to the C ABI of texgs.h (TEXGS_ABI_VERSION is unchanged); plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().
 */
#ifndef TEXGS_OPTIM_H
#define TEXGS_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_ADAM_MAX_TENSORS 32   /* records one launch carries by value in its kernel arguments */
#define TEXGS_ADAM_CHUNK 1024       /* elements one workgroup updates at a time */

/* One tensor of the step (64 bytes).  p, g, m, v are f32[numel], contiguous, 4-byte aligned, and do not overlap; they may be aligned
 * differently from each other (16-byte accesses are used when all four are 16-byte aligned).  The scalars are what the HOST has
 * already rounded to f32 from its double-precision bias corrections.  Per element, one rounding per operation, no fused multiply-add:
 *     d  = g - m;          m' = (w1 < 0.5) ? m + w1*d : g - d*(1 - w1)         (torch's lerp)
 *     v' = v*beta2;        v' = v' + (w2*g)*g
 *     den = sqrt(v')/bc2_sqrt + eps                                            (correctly rounded sqrt and divide, denormals kept)
 *     p' = p + neg_step_size*(m'/den)
 */
typedef struct TexGSAdamTensor {
    float* p;               /* parameter, updated in place */
    float* g;               /* gradient: read; written (+0.0) only with zero_grads */
    float* m;               /* exp_avg, updated in place */
    float* v;               /* exp_avg_sq, updated in place */
    int64_t numel;          /* 0: the record is skipped and its pointers may be NULL */
    float w1;               /* 1 - beta1 */
    float beta2;
    float w2;               /* 1 - beta2 */
    float bc2_sqrt;         /* sqrt(1 - beta2^step) */
    float eps;
    float neg_step_size;    /* -(lr / (1 - beta1^step)) */
} TexGSAdamTensor;

/* Steps `count` tensors: ceil(count / TEXGS_ADAM_MAX_TENSORS) launches, no copy, no temporary, no synchronisation.  zero_grads != 0
 * stores +0.0 to every g in the same pass, after it has been read.  count == 0 is a no-op.  Refused by name: count < 0, numel < 0,
 * a NULL pointer with numel > 0, a pointer that is not 4-byte aligned. */
int texgs_adam_step(const TexGSAdamTensor* tensors, int32_t count, int32_t zero_grads, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_OPTIM_H */
