/*
 * texgs_multiview.h -- the multi-view entry point of libtexgs.so (csrc/preprocess.hip): the deferred chain of the view-dependent
 * colour's gradient to the SH coefficients and to the view direction, once per multi-view step instead of once per view.
 * Additive to the C ABI of texgs.h; plain C99, nothing but <stdint.h> and <stddef.h>.
 *
 * Same conventions as texgs.h: device pointers, caller-allocated, kernels enqueued on `stream` (a hipStream_t passed as void*),
 * 0 on success, non-zero on failure with the cause in texgs_last_error().
 *
 * A backward whose TexGSGrads.dL_dvd_residue is set (texgs.h) leaves step (10) of K8 undone and stores dL/dvd -- three floats per
 * Gaussian, zero for a culled Gaussian and for a view without an active SH band -- there instead.  texgs_sh_flush does that step for
 * up to TEXGS_SH_FLUSH_MAX_VIEWS such views in one pass over the SH rows and the dL/dSH rows.
 */
#ifndef TEXGS_MULTIVIEW_H
#define TEXGS_MULTIVIEW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEXGS_SH_FLUSH_MAX_VIEWS 16   /* view records one launch carries by value in its kernel arguments */

/* One deferred view (24 bytes). */
typedef struct TexGSShFlushView {
    const float* campos;    /* f32[3], device: the view's camera position (TexGSFrame.campos of its backward) */
    const float* residue;   /* f32[N,3], device: what that backward stored through TexGSGrads.dL_dvd_residue */
    int32_t sh_degree;      /* the view's active degree, 0..3 (TexGSFrame.sh_degree); 0: the view adds nothing */
    int32_t sh_coeffs;      /* K of the backward that wrote the residue (TexGSFrame.sh_coeffs): must equal the flush's K */
} TexGSShFlushView;

/* For every Gaussian i, walking the views IN THE ORDER GIVEN, a view whose residue v = residue[i] is not all zero adds
 *     dL_dshs[i,k,c]  += b_k(dir) * v_c                   k < active coefficients of the view's degree; product rounded, then added
 *     dL_dmeans3D[i]  += (dd - dir (dir . dd)) / |d|      dd = sum_k grad b_k(dir) * (shs[i,k,:] . v),  d = means3D[i] - campos
 * with dir, the SH basis and its gradient computed by the device functions K1 and K8 use.  dL_dshs ends bit-identical to what the
 * same views' undeferred backwards accumulate in the same order (no fused multiply-add: one rounding per operation); dL_dmeans3D
 * differs from theirs in the association of one term per view.  Coefficients beyond a view's active degree get nothing from it.
 * More than TEXGS_SH_FLUSH_MAX_VIEWS views take several calls; the order of the records over the calls is the order of the sums.
 * count == 0 or N == 0 is a no-op.  Refused by name: count < 0 or above the maximum, a NULL sink / input / record pointer with
 * views pending, a degree outside 0..3, K < 1 or above 16, a record whose sh_coeffs is not K. */
int texgs_sh_flush(int32_t N, int32_t K, const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                   const TexGSShFlushView* views, int32_t count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_MULTIVIEW_H */
