/*
 * texgs_multiview.h -- the multi-view entry points of libtexgs.so: the deferred chain of the view-dependent colour's gradient to the
 * SH coefficients and to the view direction (csrc/preprocess.hip), and the batched front end, K1..K5 (csrc/preprocess.hip,
 * csrc/binning.hip) -- each once per multi-view step instead of once per view.
 * Additive to the C ABI of texgs.h, whose structs the batched front end takes; plain C99.
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

#include "texgs.h"

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

/* ---- the batched front end: K1..K5 of the views of one multi-view step in one set of launches ---------------------------------------
 * The views of a step share their Gaussians (one TexGSInputs) and differ in the camera.  Per view, K1..K5 are eleven dependent
 * launches over N Gaussians or D instances, none of which fills the chip.  The three entry points below run each of those kernels ONCE
 * for `count` views -- K1 walks the views inside the workgroup and reads the SH rows once, K2..K5 take the view as the second grid
 * dimension -- and leave in every view's TexGSGeom / TexGSBinning exactly what texgs_preprocess_forward, texgs_depth_sort_scan and the
 * K3..K5 part of texgs_bin_sort_render_forward leave there, bit for bit (the kernels' bodies are the same code).  The views' structs are
 * passed as ARRAYS of `count` elements; every view has its own buffers, sized as for the per-view calls.
 * Required: 1 <= count <= TEXGS_BATCH_MAX_VIEWS, and equal image size, num_gaussians, sh_degree, sh_coeffs and debug flag in every
 * frame -- anything else is refused by name with nothing launched, and the caller takes the per-view path. */
#define TEXGS_BATCH_MAX_VIEWS 16      /* views one launch carries by value in its kernel arguments */

/* K1 for every view.  `sums`: device u32[count * texgs_num_rendered_words(N)], view v's words at [v * words, (v + 1) * words): the
 * partial sums texgs_num_rendered_begin copies for one view, for all of them in one array -- ONE device->host copy by the caller,
 * then texgs_num_rendered_reduce per view on its slice. */
int texgs_preprocess_forward_views(const TexGSFrame* frames, const TexGSInputs* in, TexGSGeom* geoms, int32_t count, uint32_t* sums,
                                   void* stream);
/* K2 for every view (independent of D: issue it behind the copy of `sums`, it runs while the host waits). */
int texgs_depth_sort_scan_views(const TexGSGeom* geoms, int32_t num_gaussians, int32_t count, void* stream);
/* K3..K5 for every view; bins[v].num_rendered = the view's D (a view with D == 0 gets empty ranges and a tile order, as in the
 * per-view call).  Also zero-fills imgs[v].tex_bin_count where it is set, as the per-view call does: follow it with
 * texgs_render_forward_binned, not texgs_render_forward. */
int texgs_bin_sort_views(const TexGSFrame* frames, const TexGSGeom* geoms, TexGSBinning* bins, const TexGSImage* imgs, int32_t count,
                         void* stream);
/* K6 alone for ONE view whose lists texgs_bin_sort_views has just built: texgs_render_forward without its memset of tex_bin_count. */
int texgs_render_forward_binned(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom, const TexGSBinning* bin,
                                TexGSImage* img, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEXGS_MULTIVIEW_H */
