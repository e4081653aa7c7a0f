// Shared declarations for the gfx950 kernels of libtexgs.so.  CDNA4 only: wave64, 160 KiB LDS/CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "texgs.h"
#include "texgs_optim.h"
#include "texgs_multiview.h"
#include "texgs_mlp.h"
#include "texgs_present.h"
#include "texgs_ingest.h"
#include "texgs_surface.h"
#include "texgs_lpips.h"
#include "texgs_lpips_grad.h"
#include "texgs_params.h"
#include "texgs_retexture.h"
#include "texgs_shcolor.h"

// ---- operator constants (restated in oracle/texgs_torch.py) ----
#define TG_NEAR_Z        0.2f
#define TG_LOWPASS       0.3f
#define TG_FRUSTUM_CLAMP 1.3f
#define TG_ALPHA_MAX     0.99f
#define TG_ALPHA_MIN     (1.0f / 255.0f)
#define TG_T_EPS         1e-4f
#define TG_PLANE_EPS     5e-2f
#define TG_DEN_MIN       0.2f
#define TG_MA_MIN        1e-20f
#define TG_SH_C0         0.28209479177387814f

// slots of the per-Gaussian fields whose gradients K8 assembles (float index; K1 stores them split into a test and a
// shading record, texgs.h TexGSGeom)
enum {
    R_XY = 0, R_CONIC = 2, R_OP = 5, R_G2 = 6, R_GM = 8, R_PHI = 14, R_VD = 17, R_DEPTH = 20, R_N = 21
};
// accumulator-row slots (TexGSGrads.acc, 32 floats = one 128-byte line per Gaussian): raw moments about the splat centre,
// summed by K7 over the Gaussian's contributing pixels.  dx = xy - pixel, dp = pixel - xy.
//   M_P   : sum P {1, dx, dy, dx^2, dx dy, dy^2}          P = dL/dpower
//   M_DEN : sum dden {1, dpx, dpy}                         dden = dL/d(1 + g.dp)
//   M_DN  : for c = 0..2: sum dn_c {1, dpx, dpy}           dn = dL/duv / den
//   M_PHI : sum dL/duv (3)   M_VD: sum dL/dcolour (3)   M_DEPTH: sum w dL/ddepth   M_N: sum w dL/dnormal (3)
enum {
    M_P = 0, M_DEN = 6, M_DN = 9, M_PHI = 18, M_VD = 21, M_DEPTH = 24, M_N = 25
};

#define TG_BLOCK 256

struct CamConst {       // small per-frame constants passed by value in kernel args (SGPRs)
    int W, H, tiles_x, tiles_y;
    float fx, fy, tanfovx, tanfovy;
    float scale_modifier;
    int sh_degree, sh_coeffs, R, N;
};

static inline CamConst make_cam(const TexGSFrame* f) {
    CamConst c;
    c.W = f->image_width; c.H = f->image_height;
    c.tiles_x = (c.W + TEXGS_TILE - 1) / TEXGS_TILE;
    c.tiles_y = (c.H + TEXGS_TILE - 1) / TEXGS_TILE;
    c.tanfovx = f->tanfovx; c.tanfovy = f->tanfovy;
    c.fx = (float)c.W / (2.0f * f->tanfovx);
    c.fy = (float)c.H / (2.0f * f->tanfovy);
    c.scale_modifier = f->scale_modifier;
    c.sh_degree = f->sh_degree; c.sh_coeffs = f->sh_coeffs; c.R = f->tex_res; c.N = f->num_gaussians;
    return c;
}

// Status of a launcher that issues more than one runtime call: `st += hipMemsetAsync(...)` keeps the FIRST failure;
// `return st.after_launches()` adds hipGetLastError(), taken once behind the last launch (which also clears it).
struct LaunchStatus {
    hipError_t first = hipSuccess;
    void operator+=(hipError_t e) { if (first == hipSuccess) first = e; }
    hipError_t after_launches() { *this += hipGetLastError(); return first; }
};

// launchers implemented in the .hip files (host side, called from abi.hip): each returns the first failing runtime call it made,
// else hipGetLastError() behind its last launch
hipError_t launch_preprocess_fwd(const CamConst& c, const TexGSFrame* f, const TexGSInputs* in, TexGSGeom* g, hipStream_t s);
hipError_t launch_preprocess_bwd(const CamConst& c, const TexGSFrame* f, const TexGSInputs* in, const TexGSGeom* g,
                           TexGSGrads* gr, hipStream_t s);
hipError_t launch_sh_flush(int N, int K, const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                           const TexGSShFlushView* views, int count, hipStream_t s);
hipError_t launch_mark_visible(const TexGSFrame* f, const float* means3D, uint8_t* visible, hipStream_t s);
hipError_t launch_depth_sort_scan(const TexGSGeom* g, int N, hipStream_t s);
uint32_t* bin_block_sums_ptr(const TexGSGeom* g, int N);
uint32_t* bin_header_ptr(const TexGSGeom* g, int N, int* words);
size_t scan_temp_bytes(int N);
size_t sort_temp_bytes(uint32_t D, uint32_t T);
hipError_t launch_duplicate(const CamConst& c, const TexGSGeom* g, TexGSBinning* b, hipStream_t s);
hipError_t launch_sort(const CamConst& c, const TexGSGeom* g, TexGSBinning* b, hipStream_t s);
hipError_t launch_ranges(const CamConst& c, TexGSBinning* b, uint32_t* zero_words, int num_zero_words, hipStream_t s);
// the batched front end (texgs_multiview.h): arrays of `count` views, validated by the caller (abi.hip)
hipError_t launch_preprocess_fwd_views(const TexGSFrame* f, const TexGSInputs* in, TexGSGeom* g, int count, uint32_t* sums, hipStream_t s);
hipError_t launch_depth_sort_scan_views(const TexGSGeom* g, int N, int count, hipStream_t s);
hipError_t launch_bin_views(int stage, const CamConst& c, const TexGSGeom* g, const TexGSBinning* b, const TexGSImage* img, int count,
                            int num_zero_words, hipStream_t s);
hipError_t launch_render_fwd(const CamConst& c, const TexGSFrame* f, const TexGSInputs* in, const TexGSGeom* g,
                       const TexGSBinning* b, TexGSImage* img, hipStream_t s);
size_t tex_bin_count(int R);
bool tex_bins_enabled(const CamConst& c, const TexGSInputs* in, const TexGSImage* img, const TexGSGrads* gr);
hipError_t launch_texgrad_reduce(const CamConst& c, const TexGSImage* img, TexGSGrads* gr, hipStream_t s);
hipError_t launch_render_bwd(const CamConst& c, const TexGSFrame* f, const TexGSInputs* in, const TexGSGeom* g,
                       const TexGSBinning* b, const TexGSImage* img, TexGSGrads* gr, hipStream_t s);
hipError_t launch_rgb_alpha_loss(const float* image, const float* gt_image, const float* alpha, const float* gt_alpha, int H,
                          int W, float lambda_dssim, float lambda_alpha, float* scratch, float* sums, float* d_image,
                          float* d_alpha, hipStream_t s);
hipError_t launch_selftest_waveops(const float* seed128, float* out576, hipStream_t s);
hipError_t launch_geom_losses(const float* norm, const float* gt_norm, const float* gt_image, const float* mask, const float* depth,
                       const float* gt_depth, int H, int W, float lambda_norm, float lambda_smooth, float gamma,
                       float lambda_depth, float* sums, float* d_norm, float* d_depth, hipStream_t s);
hipError_t launch_norm_from_depth(const float* depth, const float* viewmatrix, float tanfovx, float tanfovy, int H, int W, float threshold,
                           float* out_norm, float* out_mask, hipStream_t s);
size_t uv_packed_bytes(int precision);          // precision: TEXGS_UV_FP32 / _BF16X3 / _MIXED, validated by the caller
hipError_t launch_uv_pack(const TexGSUVNet* net, int precision, void* packed, hipStream_t s);
hipError_t launch_uv_taylor_packed(const TexGSUVNet* net, int precision, const void* packed, const float* xyz, int N, float* uvs, float* grad_uvs,
                            hipStream_t s);
size_t uv_backward_temp_bytes(int N);
hipError_t launch_uv_backward(const TexGSUVNet* net, const float* xyz, const float* g, int N, const TexGSUVNetGrad* out, void* temp, int mixed,
                       hipStream_t s);
int hashgrid_levels(const TexGSHashGrid* g, float* scale, uint32_t* res, uint32_t* size, uint32_t* offset, uint32_t* n_params);
hipError_t launch_hashgrid_forward(const TexGSHashGrid* g, const float* params, const float* x, int N, float* enc, hipStream_t s);
size_t hashgrid_backward_temp_bytes(const TexGSHashGrid* g, int N);
hipError_t launch_hashgrid_backward(const TexGSHashGrid* g, const float* params, const float* x, const float* d_enc, int N, float* d_params,
                             float* d_x, void* temp, hipStream_t s);
size_t chamfer_nn_temp_bytes(int P);
hipError_t launch_chamfer_nn(const float* a, int P, const float* b, int Q, float* d2, int32_t* idx, void* temp, hipStream_t s);
size_t sort_pairs32_temp_bytes(uint32_t n);
hipError_t launch_sort_pairs32(const uint32_t* keys_in, uint32_t n, int key_bits, uint32_t* keys_out, uint32_t* vals_out, void* temp, hipStream_t s);
size_t knn3_temp_bytes(int n);
hipError_t launch_knn3_mean_dist2(const float* xyz, int n, float* mean_d2, void* temp, hipStream_t s);
size_t fps_temp_bytes(int n, int k);
hipError_t launch_farthest_points(const float* xyz, int n, int k, int start, int32_t* idx, void* temp, hipStream_t s);
hipError_t launch_cube_sample(const float* tex, int R, int C, const float* dirs, int N, int filter, int tap_map, float* out, hipStream_t s);
hipError_t launch_cube_latlong(const float* tex, int R, int C, int H, int W, int tap_map, float* out, hipStream_t s);
hipError_t launch_cube_sample_backward(const float* tex, int R, int C, const float* dirs, int N, const float* g_out, float* d_tex,
                                float* d_dirs, hipStream_t s);
hipError_t launch_cube_sample_nearest_backward(int R, int C, const float* dirs, int N, const float* g_out, float* d_tex, hipStream_t s);
hipError_t launch_density_stats(const float* grad, const int32_t* radii, int n, float* accum, float* denom, float* max_radii, hipStream_t s);
size_t density_plan_temp_bytes(int n);
hipError_t launch_density_plan(const TexGSDensityPlan* p, uint8_t* action, int32_t* rank, uint32_t* totals, void* temp, hipStream_t s);
hipError_t launch_density_move(const TexGSDensityMove* m, hipStream_t s);
size_t eval_metrics_temp_bytes(int H, int W);
hipError_t launch_eval_metrics(const float* image, const float* gt_image, const float* norm, const float* gt_norm, const float* alpha, int H,
                        int W, int clamp01, void* temp, double* row, hipStream_t s);
hipError_t launch_adam_step(const TexGSAdamTensor* tensors, int count, int zero_grads, hipStream_t s);
size_t mlp_param_count(const TexGSMlp* m);      // the shape is validated by the caller (abi.hip check_mlp)
size_t mlp_forward_temp_bytes();
size_t mlp_backward_temp_bytes(int N);
hipError_t launch_mlp_forward(const TexGSMlp* m, const float* params, const float* x, int N, float* y, void* temp, hipStream_t s);
hipError_t launch_mlp_backward(const TexGSMlp* m, const float* params, const float* x, const float* dy, int N, float* dx, float* d_params,
                               void* temp, hipStream_t s);
size_t depth_colour_temp_bytes(int H, int W);      // the arguments of these three are validated by the caller (abi.hip)
hipError_t launch_present(const TexGSPresent* p, hipStream_t s);
hipError_t launch_depth_colour(const TexGSDepthColour* d, void* temp, hipStream_t s);
hipError_t launch_cube_cross(const TexGSCubeCross* c, hipStream_t s);
int ingest_ksize(int inS, int outS, int filter);     // the arguments of these are validated by the caller (abi.hip)
hipError_t launch_resize_taps(int inS, int outS, int filter, int32_t* taps, int32_t* bounds, hipStream_t s);
size_t resize_temp_bytes(int H, int W, int C, int h, int w, int filter);
hipError_t launch_resize_u8(const TexGSResize* r, void* temp, hipStream_t s);
hipError_t launch_rgba_composite(const uint8_t* rgba, uint8_t* out, int H, int W, double bg0, double bg1, double bg2, hipStream_t s);
size_t surface_temp_bytes(int H, int W);             // the arguments of these are validated by the caller (abi.hip)
hipError_t launch_surface_points(const TexGSSurfacePoints* p, void* temp, hipStream_t s);
hipError_t launch_surface_compose(const TexGSSurfaceCompose* c, hipStream_t s);
size_t conv3x3_packed_bytes(int Cin, int Cout);     // the arguments of these are validated by the caller (abi.hip)
hipError_t launch_conv3x3_pack(const float* w, int Cin, int Cout, void* packed, hipStream_t s);
hipError_t launch_conv3x3(const TexGSConv3x3* d, hipStream_t s);
size_t lpips_head_temp_bytes(int P, int h, int w);
hipError_t launch_lpips_head(const TexGSLpipsHead* d, hipStream_t s);
hipError_t launch_lpips_head_backward(const TexGSLpipsHeadBackward* d, hipStream_t s);      // lpips_grad.hip, validated by abi.hip
hipError_t launch_lpips_gate(float* G, const float* y, long long n, hipStream_t s);
size_t params_temp_bytes(int32_t n);                // params.hip; the arguments of these are validated by the caller (abi.hip), n >= 1
hipError_t launch_params_activate(const TexGSParamsActivate* a, void* temp, hipStream_t s);
hipError_t launch_params_activate_backward(const TexGSParamsActivateGrad* g, hipStream_t s);
hipError_t launch_params_covariance(const TexGSParamsCovariance* c, hipStream_t s);
hipError_t launch_params_covariance_backward(const TexGSParamsCovarianceGrad* c, hipStream_t s);
hipError_t launch_retexture_cross(const TexGSRetexCross* c, hipStream_t s);        // retexture.hip, validated by abi.hip
hipError_t launch_retexture_latlong(const TexGSRetexLatLong* l, hipStream_t s);
hipError_t launch_sh_colors(const TexGSShColors* c, const TexGSShColorView* views, int count, hipStream_t s);      // shcolor.hip, validated by abi.hip
hipError_t launch_sh_colors_backward(const TexGSShColorsGrad* g, const TexGSShColorGradView* views, int count, hipStream_t s);
