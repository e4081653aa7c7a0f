// C-ABI entry points of libtexgs.so (declared in include/texgs.h).  No C++ types or exceptions cross this
// boundary: int return codes + a thread-local error string.
#include "common.h"
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

namespace {

thread_local char g_err[512] = "";

// ---- optional HIP-event kernel timing (profiling only; the data path keeps no global state) ----
struct EvRec { int kid; hipEvent_t a, b; };
std::mutex g_prof_mu;
bool g_prof_on = false;
uint32_t g_prof_mask = 0xFFFFFFFFu;       // kernel ids to bracket (an event pair costs ~5 us of stream time: bench.py brackets
                                          // only the dominant kernel inside its timed region)
std::vector<EvRec> g_prof_log;
std::vector<hipEvent_t> g_prof_free;

hipEvent_t prof_event() {   // nullptr when the runtime cannot create one: that bracket is then dropped
    if (!g_prof_free.empty()) { hipEvent_t e = g_prof_free.back(); g_prof_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}

struct ProfScope {          // brackets the launches issued inside its lifetime
    int kid; hipStream_t s; hipEvent_t a; bool on;
    ProfScope(int k, hipStream_t st) : kid(k), s(st), a(nullptr), on(false) {
        std::lock_guard<std::mutex> l(g_prof_mu);
        if (g_prof_on && ((g_prof_mask >> k) & 1u)) { a = prof_event(); on = a != nullptr; if (on) (void)hipEventRecord(a, s); }
    }
    ~ProfScope() {
        if (!on) return;
        std::lock_guard<std::mutex> l(g_prof_mu);
        hipEvent_t b = prof_event();
        if (!b) { g_prof_free.push_back(a); return; }
        (void)hipEventRecord(b, s);
        g_prof_log.push_back({kid, a, b});
    }
};

int fail(const char* where, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return (int)e ? (int)e : -1;
}

int fail_msg(const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return -1;
}

// The one place where a launcher's status (common.h) becomes a return code: a HIP error is returned as itself, with
// "<where>: <its string>" as the error text; with debug a stream sync follows (lineage `debug` semantics,
// render/uv_tex_render.py:37) and its failure is reported the same way.
int launched(const char* where, hipError_t st, hipStream_t s, bool debug) {
    if (st == hipSuccess && debug) st = hipStreamSynchronize(s);
    return st == hipSuccess ? 0 : fail(where, st);
}

int validate_frame(const TexGSFrame* f) {
    if (!f) return fail_msg("frame is NULL");
    if (f->image_height <= 0 || f->image_width <= 0) return fail_msg("image size must be positive");
    if (f->image_width > 65535 * TEXGS_TILE || f->image_height > 65535 * TEXGS_TILE) return fail_msg("image too large");
    {   // tile ids are sorted in at most three 8-bit digits and live in the high word of a 64-bit key
        const long long tx = (f->image_width + TEXGS_TILE - 1) / TEXGS_TILE, ty = (f->image_height + TEXGS_TILE - 1) / TEXGS_TILE;
        if (tx * ty > (1ll << 24)) return fail_msg("image too large: more than 2^24 tiles");
    }
    if (f->sh_degree < 0 || f->sh_degree > 3) return fail_msg("sh_degree must be in [0,3]");
    if (f->num_gaussians < 0) return fail_msg("num_gaussians < 0");
    if (f->tex_res <= 0) return fail_msg("tex_res must be positive");
    if (f->tex_res > 7168) return fail_msg("tex_res > 7168: the blend kernels address texels with 32-bit byte offsets (6 R^2 x 12 B < 2^32)");
    if (!f->bg || !f->viewmatrix || !f->projmatrix || !f->campos) return fail_msg("frame device pointers must be non-NULL");
    return 0;
}

}  // namespace

extern "C" {

int texgs_abi_version(void) { return TEXGS_ABI_VERSION; }

#ifndef TEXGS_BUILD_ID
#define TEXGS_BUILD_ID "unknown"
#endif
const char* texgs_build_id(void) { return TEXGS_BUILD_ID; }

const char* texgs_last_error(void) { return g_err; }

size_t texgs_scan_temp_bytes(int32_t num_gaussians) { return scan_temp_bytes(num_gaussians); }

size_t texgs_sort_temp_bytes(uint32_t num_rendered, uint32_t num_tiles) { return sort_temp_bytes(num_rendered, num_tiles); }

size_t texgs_tex_bin_count(int32_t tex_res) { return tex_bin_count(tex_res); }

int texgs_preprocess_forward(const TexGSFrame* frame, const TexGSInputs* in, TexGSGeom* geom, void* stream) {
    if (int r = validate_frame(frame)) return r;
    if (!in || !geom) return fail_msg("NULL argument");
    if (frame->num_gaussians == 0) return 0;
    if (!in->means3D || !in->opacities) return fail_msg("per-Gaussian input pointer is NULL");
    if (in->texture && (!in->uvs || !in->gradient_uvs)) return fail_msg("uvs / gradient_uvs are required with a texture");
    if (in->cov3D_precomp && in->texture) return fail_msg("cov3D_precomp is an input of the untextured surface only (texture must be NULL)");
    if (!in->cov3D_precomp && (!in->scales || !in->rotations)) return fail_msg("scales and rotations (or cov3D_precomp) are required");
    if (geom->scan_temp_bytes < scan_temp_bytes(frame->num_gaussians)) return fail_msg("scan_temp too small");
    hipStream_t s = (hipStream_t)stream;
    const CamConst c = make_cam(frame);
    hipError_t st;
    { ProfScope p(TEXGS_K_PREPROCESS_FWD, s); st = launch_preprocess_fwd(c, frame, in, geom, s); }
    return launched("preprocess_fwd", st, s, frame->debug);
}

// K2: depth sort of the Gaussians + exclusive scan of tiles_touched in depth-rank order (independent of D)
static int depth_sort_scan(const TexGSGeom* geom, int32_t num_gaussians, hipStream_t s, bool debug) {
    if (num_gaussians == 0) return 0;
    hipError_t st;
    { ProfScope p(TEXGS_K_SCAN, s); st = launch_depth_sort_scan(geom, num_gaussians, s); }
    return launched("depth sort / scan", st, s, debug);
}

// D = sum of tiles_touched and the geometry fingerprint, read back in two steps so that a caller can issue K1 of a LATER view early
// (texgs.rasterizer forward prefetch): `begin` copies K1's per-workgroup partial sums (three per workgroup; no atomics, nothing to
// zero-fill) into the caller's PINNED host buffer asynchronously and, with sort_first, launches K2 -- depth sort + scan, which WRITE
// geom->offsets and geom->scan_temp -- so the device stays busy during the sync; the caller records an event of its own behind it and
// goes on; `reduce` -- host only, after that event has completed -- adds them up.
size_t texgs_num_rendered_words(int32_t num_gaussians) {
    return num_gaussians <= 0 ? 0 : 3 * (((size_t)num_gaussians + TG_BLOCK - 1) / TG_BLOCK);
}
int texgs_num_rendered_begin(const TexGSGeom* geom, int32_t num_gaussians, uint32_t* host_pinned, size_t host_words, int32_t sort_first,
                             void* stream) {
    if (!geom || !host_pinned) return fail_msg("NULL argument");
    if (num_gaussians <= 0) return 0;
    const size_t nw = texgs_num_rendered_words(num_gaussians);
    if (host_words < nw) return fail_msg("host buffer too small (texgs_num_rendered_words)");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(host_pinned, bin_block_sums_ptr(geom, num_gaussians), nw * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return fail("num_rendered readback", e);
    return sort_first ? depth_sort_scan(geom, num_gaussians, s, false) : 0;
}
int texgs_num_rendered_reduce(const uint32_t* host_pinned, int32_t num_gaussians, uint32_t* host_out, uint64_t* fingerprint_out) {
    if (!host_pinned || !host_out) return fail_msg("NULL argument");
    *host_out = 0;
    if (fingerprint_out) *fingerprint_out = 0;
    if (num_gaussians <= 0) return 0;
    const size_t nblk = ((size_t)num_gaussians + TG_BLOCK - 1) / TG_BLOCK;
    unsigned long long total = 0ull;
    uint32_t fa = 0u, fb = 0u;
    for (size_t k = 0; k < nblk; ++k) { total += host_pinned[k]; fa += host_pinned[nblk + k]; fb += host_pinned[2 * nblk + k]; }
    if (total > 0xFFFFFFFFull) return fail_msg("num_rendered exceeds 2^32 - 1 instances");
    *host_out = (uint32_t)total;
    if (fingerprint_out) *fingerprint_out = ((uint64_t)fb << 32) | (uint64_t)fa;
    return 0;
}

int texgs_depth_sort_scan(TexGSGeom* geom, int32_t num_gaussians, void* stream) {
    if (!geom) return fail_msg("NULL argument");
    return depth_sort_scan(geom, num_gaussians, (hipStream_t)stream, false);
}

static int render_forward_impl(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom,
                               const TexGSBinning* bin, TexGSImage* img, void* stream, bool counters_zeroed) {
    if (int r = validate_frame(frame)) return r;
    if (!in || !geom || !bin || !img) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const CamConst c = make_cam(frame);
    if (img->tex_bin_count && in->texture && !counters_zeroed) {       // K6 counts the texture-gradient footprints per bin into it
        hipError_t e = hipMemsetAsync(img->tex_bin_count, 0, sizeof(uint32_t) * 2 * tex_bin_count(c.R), s);
        if (e != hipSuccess) return fail("tex_bin_count memset", e);
    }
    hipError_t st;
    { ProfScope p(TEXGS_K_RENDER_FWD, s); st = launch_render_fwd(c, frame, in, geom, bin, img, s); }
    return launched("render_fwd", st, s, frame->debug);
}

int texgs_render_forward(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom,
                         const TexGSBinning* bin, TexGSImage* img, void* stream) {
    return render_forward_impl(frame, in, geom, bin, img, stream, false);
}

int texgs_bin_sort_render_forward(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom,
                                  TexGSBinning* bin, TexGSImage* img, void* stream) {
    if (int r = validate_frame(frame)) return r;
    if (!in || !geom || !bin || !img) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    const CamConst c = make_cam(frame);
    hipError_t st;
    if (bin->num_rendered > 0) {
        if (bin->sort_temp_bytes < sort_temp_bytes(bin->num_rendered, (uint32_t)(c.tiles_x * c.tiles_y))) return fail_msg("sort_temp too small");
        { ProfScope p(TEXGS_K_DUPLICATE, s); st = launch_duplicate(c, geom, bin, s); }
        if (int r = launched("duplicate_with_keys", st, s, frame->debug)) return r;
        { ProfScope p(TEXGS_K_SORT, s); st = launch_sort(c, geom, bin, s); }
        if (int r = launched("tile sort", st, s, frame->debug)) return r;
    }
    // (the one-workgroup tile-order kernel also zero-fills the per-bin footprint counters K6 adds into)
    { ProfScope p(TEXGS_K_RANGES, s);
      st = launch_ranges(c, bin, img->tex_bin_count, img->tex_bin_count ? 2 * (int)tex_bin_count(c.R) : 0, s); }
    if (int r = launched("tile_ranges", st, s, frame->debug)) return r;
    return render_forward_impl(frame, in, geom, bin, img, stream, true);
}

int texgs_backward_render(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom,
                          const TexGSBinning* bin, const TexGSImage* img, TexGSGrads* grads, void* stream) {
    if (int r = validate_frame(frame)) return r;
    if (!in || !geom || !bin || !img || !grads) return fail_msg("NULL argument");
    if (!(grads->want & TEXGS_WANT_ALL)) return fail_msg("TexGSGrads.want is empty: ask for TEXGS_WANT_TEXTURE and / or TEXGS_WANT_GAUSSIANS");
    if ((grads->want & TEXGS_WANT_GAUSSIANS) && !grads->acc) return fail_msg("acc must be allocated (zero-filled) when Gaussian gradients are wanted");
    if ((grads->want & TEXGS_WANT_TEXTURE) && in->texture && !grads->dL_dtexture) return fail_msg("dL_dtexture must be allocated (zero-filled) when the texture gradient is wanted");
    if (!img->survivors || !img->surv_qmask || !img->surv_count)
        return fail_msg("the forward of this call left no survivor lists (TexGSImage.survivors / surv_qmask / surv_count were NULL): "
                        "run the forward with them to be able to run its backward");
    hipStream_t s = (hipStream_t)stream;
    const CamConst c = make_cam(frame);
    if (bin->num_rendered > 0) {
        hipError_t st;
        { ProfScope p(TEXGS_K_RENDER_BWD, s); st = launch_render_bwd(c, frame, in, geom, bin, img, grads, s); }
        if (int r = launched("render_bwd", st, s, frame->debug)) return r;
        if (tex_bins_enabled(c, in, img, grads)) {
            { ProfScope p(TEXGS_K_TEXGRAD_REDUCE, s); st = launch_texgrad_reduce(c, img, grads, s); }
            return launched("texgrad_reduce", st, s, frame->debug);
        }
    }
    return 0;
}

int texgs_backward_preprocess(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom, TexGSGrads* grads,
                              void* stream) {
    if (int r = validate_frame(frame)) return r;
    if (!in || !geom || !grads) return fail_msg("NULL argument");
    if (!(grads->want & TEXGS_WANT_GAUSSIANS)) return 0;          // nobody reads a per-Gaussian gradient: K7 summed no moments either
    if (!grads->acc) return fail_msg("acc must be allocated");
    if (in->cov3D_precomp && !grads->dL_dcov3D) return fail_msg("dL_dcov3D is required with cov3D_precomp");
    if (grads->dL_dvd_residue && (grads->accumulate & (TEXGS_ACC_SHS | TEXGS_ACC_MEANS3D)) != (TEXGS_ACC_SHS | TEXGS_ACC_MEANS3D))
        return fail_msg("dL_dvd_residue needs TEXGS_ACC_SHS and TEXGS_ACC_MEANS3D in accumulate: texgs_sh_flush adds into both");
    hipStream_t s = (hipStream_t)stream;
    const CamConst c = make_cam(frame);
    hipError_t st;
    { ProfScope p(TEXGS_K_PREPROCESS_BWD, s); st = launch_preprocess_bwd(c, frame, in, geom, grads, s); }
    return launched("preprocess_bwd", st, s, frame->debug);
}

// (Round 5, measured null: the texture-gradient reduce on a side stream next to K8 -- both wait only for K7 -- changed nothing:
// reference call pattern 728.0 vs 728.2 and 720.7 vs 712.5 views/s, iteration leg 5.172 vs 5.170 ms, profiles/r05_ablation.md.)
int texgs_backward(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom,
                   const TexGSBinning* bin, const TexGSImage* img, TexGSGrads* grads, void* stream) {
    if (int r = texgs_backward_render(frame, in, geom, bin, img, grads, stream)) return r;
    return texgs_backward_preprocess(frame, in, geom, grads, stream);
}

int texgs_profile_enable(int on) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    g_prof_on = on != 0;
    if (!g_prof_on) {
        for (auto& r : g_prof_log) { g_prof_free.push_back(r.a); g_prof_free.push_back(r.b); }
        g_prof_log.clear();
    }
    return 0;
}

int texgs_profile_select(uint32_t kernel_mask) {
    std::lock_guard<std::mutex> l(g_prof_mu);
    g_prof_mask = kernel_mask;
    return 0;
}

int texgs_profile_read(float* ms_sum_host, uint32_t* launches_host) {
    if (!ms_sum_host || !launches_host) return fail_msg("NULL argument");
    std::lock_guard<std::mutex> l(g_prof_mu);
    for (auto& r : g_prof_log) {
        hipError_t e = hipEventSynchronize(r.b);
        if (e != hipSuccess) return fail("profile event sync", e);
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, r.a, r.b);
        if (e != hipSuccess) return fail("profile elapsed", e);
        if (r.kid >= 0 && r.kid < TEXGS_NUM_KERNELS) { ms_sum_host[r.kid] += ms; launches_host[r.kid] += 1; }
        g_prof_free.push_back(r.a); g_prof_free.push_back(r.b);
    }
    g_prof_log.clear();
    return 0;
}

int texgs_rgb_alpha_loss(const float* image, const float* gt_image, const float* alpha, const float* gt_alpha,
                         int32_t H, int32_t W, float lambda_dssim, float lambda_alpha, float* scratch, float* sums,
                         float* dL_dimage, float* dL_dalpha, void* stream) {
    if (!image || !gt_image || !scratch || !sums || !dL_dimage) return fail_msg("NULL argument");
    if (H <= 0 || W <= 0) return fail_msg("image size must be positive");
    hipStream_t s = (hipStream_t)stream;
    return launched("rgb_alpha_loss", launch_rgb_alpha_loss(image, gt_image, alpha, gt_alpha, H, W, lambda_dssim, lambda_alpha, scratch,
                                                            sums, dL_dimage, dL_dalpha, s), s, false);
}

int texgs_geom_losses(const float* norm, const float* gt_norm, const float* gt_image, const float* mask, const float* depth,
                      const float* gt_depth, int32_t H, int32_t W, float lambda_norm, float lambda_smooth, float gamma,
                      float lambda_depth, float* sums, float* dL_dnorm, float* dL_ddepth, void* stream) {
    if (!sums) return fail_msg("NULL argument");
    if (H <= 0 || W <= 0 || !(gamma > 0.f)) return fail_msg("image size and gamma must be positive");
    if (lambda_norm != 0.f && (!norm || !gt_norm || !dL_dnorm)) return fail_msg("norm term needs norm, gt_norm, dL_dnorm");
    if (lambda_smooth != 0.f && (!norm || !gt_image || !dL_dnorm)) return fail_msg("smoothness term needs norm, gt_image, dL_dnorm");
    if (lambda_depth != 0.f && (!depth || !gt_depth || !dL_ddepth)) return fail_msg("depth term needs depth, gt_depth, dL_ddepth");
    hipStream_t s = (hipStream_t)stream;
    return launched("geom_losses", launch_geom_losses(norm, gt_norm, gt_image, mask, depth, gt_depth, H, W, lambda_norm, lambda_smooth,
                                                      gamma, lambda_depth, sums, dL_dnorm, dL_ddepth, s), s, false);
}

int texgs_norm_from_depth(const float* depth, const float* viewmatrix, float tanfovx, float tanfovy, int32_t H, int32_t W,
                          float threshold, float* out_norm, float* out_mask, void* stream) {
    if (!depth || !viewmatrix || !out_norm || !out_mask) return fail_msg("NULL argument");
    if (H <= 0 || W <= 0) return fail_msg("image size must be positive");
    hipStream_t s = (hipStream_t)stream;
    return launched("norm_from_depth", launch_norm_from_depth(depth, viewmatrix, tanfovx, tanfovy, H, W, threshold, out_norm, out_mask, s),
                    s, false);
}

static int check_uvnet(const TexGSUVNet* net, int32_t precision) {
    if (precision != TEXGS_UV_FP32 && precision != TEXGS_UV_BF16X3 && precision != TEXGS_UV_MIXED)
        return fail_msg("precision must be TEXGS_UV_FP32, TEXGS_UV_BF16X3 or TEXGS_UV_MIXED");
    if (net->hidden != 128) return fail_msg("the UV-map kernels support the shipped UVNet shape only (hidden width 128)");
    if (!net->W1 || !net->W2 || !net->W3 || !net->W4 || !net->W5 || !net->emb) return fail_msg("weight pointer is NULL");
    return 0;
}

size_t texgs_uv_packed_bytes(int32_t precision) { return uv_packed_bytes(precision); }

int texgs_uv_pack(const TexGSUVNet* net, int32_t precision, void* packed, void* stream) {
    if (!net || !packed) return fail_msg("NULL argument");
    if (int r = check_uvnet(net, precision)) return r;
    hipStream_t s = (hipStream_t)stream;
    return launched("uv_pack", launch_uv_pack(net, precision, packed, s), s, false);
}

int texgs_uv_taylor_packed(const TexGSUVNet* net, int32_t precision, const void* packed, const float* xyz, int32_t N, float* uvs,
                           float* grad_uvs, void* stream) {
    if (!net || !packed) return fail_msg("NULL argument");
    if (int r = check_uvnet(net, precision)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (N > 0 && (!xyz || !uvs || !grad_uvs)) return fail_msg("NULL argument");   /* (an empty tensor's data pointer is NULL) */
    hipStream_t s = (hipStream_t)stream;
    return launched("uv_taylor", launch_uv_taylor_packed(net, precision, packed, xyz, N, uvs, grad_uvs, s), s, false);
}

size_t texgs_uv_backward_temp_bytes(int32_t N) { return uv_backward_temp_bytes(N < 0 ? 0 : N); }

int texgs_uv_backward(const TexGSUVNet* net, int32_t precision, const float* xyz, const float* g_uvs, int32_t N, const TexGSUVNetGrad* out,
                      void* temp, void* stream) {
    if (!net || !out || !temp) return fail_msg("NULL argument");
    if (int r = check_uvnet(net, precision)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (N > 0 && (!xyz || !g_uvs)) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("uv_backward", launch_uv_backward(net, xyz, g_uvs, N, out, temp, precision != TEXGS_UV_FP32, s), s, false);
}

static int check_hashgrid(const TexGSHashGrid* g, uint32_t* n_params) {
    if (!g) return fail_msg("grid is NULL");
    float sc[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t r[TEXGS_HASHGRID_MAX_LEVELS], sz[TEXGS_HASHGRID_MAX_LEVELS], off[TEXGS_HASHGRID_MAX_LEVELS];
    switch (hashgrid_levels(g, sc, r, sz, off, n_params)) {
    case 0: return 0;
    case -1: return fail_msg("hash grid: n_levels must be in [1, 16]");
    case -2: return fail_msg("hash grid: n_features must be 4");
    case -3: return fail_msg("hash grid: log2_hashmap_size must be in [1, 24]");
    case -4: return fail_msg("hash grid: base_resolution must be >= 1 and per_level_scale in [1, 16]");
    case -5: return fail_msg("hash grid: a level's resolution is out of range");
    default: return fail_msg("hash grid: more than 2^31 parameters");
    }
}

int texgs_hashgrid_levels(const TexGSHashGrid* grid, float* scale, uint32_t* res, uint32_t* size, uint32_t* offset, uint32_t* n_params) {
    uint32_t n = 0;
    if (int r = check_hashgrid(grid, &n)) return r;
    float sc[TEXGS_HASHGRID_MAX_LEVELS];
    uint32_t rs[TEXGS_HASHGRID_MAX_LEVELS], sz[TEXGS_HASHGRID_MAX_LEVELS], off[TEXGS_HASHGRID_MAX_LEVELS];
    hashgrid_levels(grid, sc, rs, sz, off, &n);
    for (int l = 0; l < grid->n_levels; ++l) {
        if (scale) scale[l] = sc[l];
        if (res) res[l] = rs[l];
        if (size) size[l] = sz[l];
        if (offset) offset[l] = off[l];
    }
    if (n_params) *n_params = n;
    return 0;
}

int texgs_hashgrid_forward(const TexGSHashGrid* grid, const float* params, const float* x, int32_t N, float* enc, void* stream) {
    uint32_t n = 0;
    if (int r = check_hashgrid(grid, &n)) return r;
    if (N < 0) return fail_msg("N < 0");
    if ((int64_t)N * grid->n_levels * TEXGS_HASHGRID_FEATURES > INT32_MAX) return fail_msg("N * L * F >= 2^31");
    if (N > 0 && (!params || !x || !enc)) return fail_msg("NULL argument");
    if (N > 0 && (((uintptr_t)params | (uintptr_t)enc) & 15)) return fail_msg("params and enc must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("hashgrid_forward", launch_hashgrid_forward(grid, params, x, N, enc, s), s, false);
}

size_t texgs_hashgrid_backward_temp_bytes(const TexGSHashGrid* grid, int32_t N) {
    uint32_t n = 0;
    if (!grid || check_hashgrid(grid, &n)) return 0;
    return hashgrid_backward_temp_bytes(grid, N);
}

int texgs_hashgrid_backward(const TexGSHashGrid* grid, const float* params, const float* x, const float* d_enc, int32_t N,
                            float* d_params, float* d_x, void* temp, void* stream) {
    uint32_t n = 0;
    if (int r = check_hashgrid(grid, &n)) return r;
    if (N < 0) return fail_msg("N < 0");
    if ((int64_t)N * grid->n_levels * TEXGS_HASHGRID_FEATURES > INT32_MAX) return fail_msg("N * L * F >= 2^31");
    if (N > 0 && (!params || !x || !d_enc)) return fail_msg("NULL argument");
    if (N > 0 && (((uintptr_t)params | (uintptr_t)d_enc | (uintptr_t)d_params) & 15))
        return fail_msg("params, d_enc and d_params must be 16-byte aligned");
    if (N > 0 && d_x && !temp) return fail_msg("temp is NULL (d_x needs texgs_hashgrid_backward_temp_bytes)");
    hipStream_t s = (hipStream_t)stream;
    return launched("hashgrid_backward", launch_hashgrid_backward(grid, params, x, d_enc, N, d_params, d_x, temp, s), s, false);
}

size_t texgs_chamfer_nn_temp_bytes(int32_t P) { return chamfer_nn_temp_bytes(P); }

int texgs_chamfer_nn(const float* a, int32_t P, const float* b, int32_t Q, float* d2, int32_t* idx, void* temp, void* stream) {
    if (P < 0) return fail_msg("P < 0");
    if (Q < 1) return fail_msg("the reference set is empty (Q < 1)");
    if ((int64_t)Q > 65535ll * 512) return fail_msg("Q > 65535 * 512");
    if (P > 0 && (!a || !b || !d2 || !idx || !temp)) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("chamfer_nn", launch_chamfer_nn(a, P, b, Q, d2, idx, temp, s), s, false);
}

size_t texgs_knn3_temp_bytes(int32_t n) { return knn3_temp_bytes(n); }

int texgs_knn3_mean_dist2(const float* xyz, int32_t n, float* mean_d2, void* temp, void* stream) {
    if (n < 4) return fail_msg("n < 4: three nearest other points need at least four points");
    if (!xyz || !mean_d2 || !temp) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("knn3_mean_dist2", launch_knn3_mean_dist2(xyz, n, mean_d2, temp, s), s, false);
}

size_t texgs_fps_temp_bytes(int32_t n, int32_t k) { return fps_temp_bytes(n, k); }

int texgs_farthest_points(const float* xyz, int32_t n, int32_t k, int32_t start, int32_t* idx, void* temp, void* stream) {
    if (n < 1) return fail_msg("n < 1");
    if (k < 1 || k > n) return fail_msg("k must be in [1, n]");
    if (start < 0 || start >= n) return fail_msg("start must be in [0, n)");
    if (!xyz || !idx || !temp) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("farthest_points", launch_farthest_points(xyz, n, k, start, idx, temp, s), s, false);
}

static int cube_shape_ok(int32_t R, int32_t C) {
    if (R < 2) return fail_msg("R < 2: a cubemap face needs at least 2 x 2 texels");
    if (C < 1) return fail_msg("C < 1");
    if (6ll * R * R * C >= (1ll << 31)) return fail_msg("6 R R C must be below 2^31");
    return 0;
}

int texgs_cube_sample(const float* tex, int32_t R, int32_t C, const float* dirs, int32_t N, int32_t filter, int32_t tap_map,
                      float* out, void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (filter != TEXGS_CUBE_LINEAR && filter != TEXGS_CUBE_NEAREST) return fail_msg("filter must be TEXGS_CUBE_LINEAR or TEXGS_CUBE_NEAREST");
    if (!tex || (N > 0 && (!dirs || !out))) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_sample", launch_cube_sample(tex, R, C, dirs, N, filter, tap_map, out, s), s, false);
}

int texgs_cube_latlong(const float* tex, int32_t R, int32_t C, int32_t H, int32_t W, int32_t tap_map, float* out, void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (H < 1 || W < 1) return fail_msg("H and W must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("H W must be below 2^31");
    if (!tex || !out) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_latlong", launch_cube_latlong(tex, R, C, H, W, tap_map, out, s), s, false);
}

int texgs_cube_sample_backward(const float* tex, int32_t R, int32_t C, const float* dirs, int32_t N, const float* g_out,
                               float* d_tex, float* d_dirs, void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (!d_tex && !d_dirs) return fail_msg("d_tex and d_dirs are both NULL: nothing to compute");
    if ((d_dirs && !tex) || (N > 0 && (!dirs || !g_out))) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_sample_backward", launch_cube_sample_backward(tex, R, C, dirs, N, g_out, d_tex, d_dirs, s), s, false);
}

int texgs_cube_sample_nearest_backward(int32_t R, int32_t C, const float* dirs, int32_t N, const float* g_out, float* d_tex,
                                       void* stream) {
    if (int r = cube_shape_ok(R, C)) return r;
    if (N < 0) return fail_msg("N < 0");
    if (!d_tex || (N > 0 && (!dirs || !g_out))) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_sample_nearest_backward", launch_cube_sample_nearest_backward(R, C, dirs, N, g_out, d_tex, s), s, false);
}

int texgs_density_stats(const float* grad, const int32_t* radii, int32_t n, float* accum, float* denom, float* max_radii, void* stream) {
    if (n < 0) return fail_msg("n < 0");
    if (n > 0 && (!grad || !radii || !accum || !denom || !max_radii)) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("density_stats", launch_density_stats(grad, radii, n, accum, denom, max_radii, s), s, false);
}

size_t texgs_density_plan_temp_bytes(int32_t n) { return density_plan_temp_bytes(n); }

int texgs_density_plan(const TexGSDensityPlan* plan, uint8_t* action, int32_t* rank, uint32_t* totals, void* temp, void* stream) {
    if (!plan || !totals) return fail_msg("NULL argument");
    if (plan->n < 0) return fail_msg("n < 0");
    if (plan->n > 0 && (!plan->scaling || !plan->opacity || !action || !rank || !temp)) return fail_msg("NULL argument");
    if (plan->n > 0 && plan->densify && (!plan->accum || !plan->denom)) return fail_msg("accum and denom are required to densify");
    if (plan->densify && !(plan->max_grad > 0.0f)) return fail_msg("max_grad must be positive (with 0 the reference splits its own clones)");
    hipStream_t s = (hipStream_t)stream;
    return launched("density_plan", launch_density_plan(plan, action, rank, totals, temp, s), s, false);
}

int texgs_density_move(const TexGSDensityMove* m, void* stream) {
    if (!m) return fail_msg("NULL argument");
    if (m->n < 0 || m->n_kept < 0 || m->n_clone < 0 || m->n_split < 0 || m->n_child < 0) return fail_msg("negative count");
    if (m->n_kept > m->n || m->n_clone > m->n || m->n_split > m->n || m->n_child > m->n_split) return fail_msg("totals exceed n");
    if ((int64_t)m->n_kept + m->n_clone + 2ll * m->n_child >= (1ll << 31)) return fail_msg("the new row count reaches 2^31");
    if (m->rows < 0 || m->rows > TEXGS_DENSITY_MAX_ROWS) return fail_msg("rows must be in [0, TEXGS_DENSITY_MAX_ROWS]");
    if (m->n == 0 || m->rows == 0) return 0;
    if (!m->action || !m->rank) return fail_msg("NULL argument");
    const bool out_rows = m->n_kept + m->n_clone + m->n_child > 0;
    for (int d = 0; d < m->rows; ++d) {
        const TexGSDensityRow& r = m->row[d];
        if (r.width < 1) return fail_msg("row width < 1");
        if (r.kind < TEXGS_DENSITY_ROW_COPY || r.kind > TEXGS_DENSITY_ROW_XYZ) return fail_msg("unknown row kind");
        if (r.kind == TEXGS_DENSITY_ROW_XYZ && r.width != 3) return fail_msg("an XYZ row has width 3");
        if (!r.src || (out_rows && !r.dst)) return fail_msg("NULL row pointer");
        if (r.kind == TEXGS_DENSITY_ROW_XYZ && m->n_child > 0 && (!m->scaling || !m->rotation || !m->noise))
            return fail_msg("an XYZ row with children needs scaling, rotation and noise");
    }
    if (!out_rows) return 0;        // everything pruned: there is no row to write
    return launched("density_move", launch_density_move(m, (hipStream_t)stream), (hipStream_t)stream, false);
}

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

// include/texgs_optim.h: every record is checked before the first launch, so a refused call has changed nothing
int texgs_adam_step(const TexGSAdamTensor* tensors, int32_t count, int32_t zero_grads, void* stream) {
    if (count < 0) return fail_msg("count < 0");
    if (count == 0) return 0;
    if (!tensors) return fail_msg("tensors is NULL");
    for (int32_t k = 0; k < count; ++k) {
        const TexGSAdamTensor& t = tensors[k];
        if (t.numel < 0) return fail_msg("numel < 0");
        if (t.numel == 0) continue;
        if (!t.p || !t.g || !t.m || !t.v) return fail_msg("NULL pointer (p, g, m or v) in a record with numel > 0");
        if (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3)
            return fail_msg("p, g, m and v must be 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    for (int32_t first = 0; first < count; first += TEXGS_ADAM_MAX_TENSORS) {
        const int32_t n = count - first < TEXGS_ADAM_MAX_TENSORS ? count - first : TEXGS_ADAM_MAX_TENSORS;
        if (int r = launched("adam_step", launch_adam_step(tensors + first, n, zero_grads, s), s, false)) return r;
    }
    return 0;
}

// include/texgs_multiview.h: every record is checked before the launch, so a refused call has changed nothing
int texgs_sh_flush(int32_t N, int32_t K, const float* means3D, const float* shs, float* dL_dshs, float* dL_dmeans3D,
                   const TexGSShFlushView* views, int32_t count, void* stream) {
    if (count < 0) return fail_msg("count < 0");
    if (count > TEXGS_SH_FLUSH_MAX_VIEWS) return fail_msg("count exceeds TEXGS_SH_FLUSH_MAX_VIEWS: flush in several calls");
    if (N < 0) return fail_msg("N < 0");
    if (count == 0 || N == 0) return 0;
    if (!dL_dshs || !dL_dmeans3D) return fail_msg("NULL sink (dL_dshs or dL_dmeans3D) with views pending");
    if (!means3D || !shs || !views) return fail_msg("NULL argument (means3D, shs or views) with views pending");
    if (K < 1 || K > 16) return fail_msg("K must be in [1,16]");
    for (int32_t k = 0; k < count; ++k) {
        const TexGSShFlushView& v = views[k];
        if (!v.campos || !v.residue) return fail_msg("NULL campos or residue in a view record");
        if (v.sh_degree < 0 || v.sh_degree > 3) return fail_msg("sh_degree of a view record must be in [0,3]");
        if (v.sh_coeffs != K) {
            snprintf(g_err, sizeof(g_err), "K does not match: view %d wrote its residue with K = %d, the flush has K = %d", (int)k,
                     (int)v.sh_coeffs, (int)K);
            return -1;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    return launched("sh_flush", launch_sh_flush(N, K, means3D, shs, dL_dshs, dL_dmeans3D, views, count, s), s, false);
}

// include/texgs_multiview.h, the batched front end: what the views of one batch must share, by name; nothing is launched on a refusal
static int check_views(const TexGSFrame* frames, int32_t count) {
    if (!frames) return fail_msg("frames is NULL");
    if (count < 1) return fail_msg("count < 1");
    if (count > TEXGS_BATCH_MAX_VIEWS) return fail_msg("count exceeds TEXGS_BATCH_MAX_VIEWS: batch in several calls or take the per-view path");
    for (int32_t v = 0; v < count; ++v) {
        if (int r = validate_frame(&frames[v])) return r;
        const TexGSFrame &a = frames[0], &b = frames[v];
        if (a.image_height != b.image_height || a.image_width != b.image_width) return fail_msg("the views of a batch must have one image size");
        if (a.num_gaussians != b.num_gaussians) return fail_msg("the views of a batch must have one num_gaussians");
        if (a.sh_degree != b.sh_degree || a.sh_coeffs != b.sh_coeffs) return fail_msg("the views of a batch must have one sh_degree and one sh_coeffs");
        if ((a.debug != 0) != (b.debug != 0)) return fail_msg("the views of a batch must have one debug flag");
    }
    if (frames[0].num_gaussians == 0) return fail_msg("num_gaussians == 0: nothing to batch, take the per-view path");
    return 0;
}

int texgs_preprocess_forward_views(const TexGSFrame* frames, const TexGSInputs* in, TexGSGeom* geoms, int32_t count, uint32_t* sums,
                                   void* stream) {
    if (int r = check_views(frames, count)) return r;
    if (!in || !geoms || !sums) return fail_msg("NULL argument");
    if (!in->means3D || !in->opacities) return fail_msg("per-Gaussian input pointer is NULL");
    if (in->texture && (!in->uvs || !in->gradient_uvs)) return fail_msg("uvs / gradient_uvs are required with a texture");
    if (in->cov3D_precomp && in->texture) return fail_msg("cov3D_precomp is an input of the untextured surface only (texture must be NULL)");
    if (!in->cov3D_precomp && (!in->scales || !in->rotations)) return fail_msg("scales and rotations (or cov3D_precomp) are required");
    for (int32_t v = 0; v < count; ++v) {
        const TexGSGeom& g = geoms[v];
        if (!g.rec_test || !g.rec_shade || !g.depth || !g.radii || !g.rect || !g.tiles_touched || !g.scan_temp) return fail_msg("NULL buffer in a view's TexGSGeom");
        if (g.scan_temp_bytes < scan_temp_bytes(frames[0].num_gaussians)) return fail_msg("scan_temp too small");
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t st;
    { ProfScope p(TEXGS_K_PREPROCESS_FWD, s); st = launch_preprocess_fwd_views(frames, in, geoms, count, sums, s); }
    return launched("preprocess_fwd (views)", st, s, frames[0].debug);
}

int texgs_depth_sort_scan_views(const TexGSGeom* geoms, int32_t num_gaussians, int32_t count, void* stream) {
    if (!geoms) return fail_msg("NULL argument");
    if (count < 1 || count > TEXGS_BATCH_MAX_VIEWS) return fail_msg("count must be in [1, TEXGS_BATCH_MAX_VIEWS]");
    if (num_gaussians <= 0) return fail_msg("num_gaussians must be positive");
    for (int32_t v = 0; v < count; ++v) {
        if (!geoms[v].depth || !geoms[v].tiles_touched || !geoms[v].scan_temp) return fail_msg("NULL buffer in a view's TexGSGeom");
        if (geoms[v].scan_temp_bytes < scan_temp_bytes(num_gaussians)) return fail_msg("scan_temp too small");
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t st;
    { ProfScope p(TEXGS_K_SCAN, s); st = launch_depth_sort_scan_views(geoms, num_gaussians, count, s); }
    return launched("depth sort / scan (views)", st, s, false);
}

int texgs_bin_sort_views(const TexGSFrame* frames, const TexGSGeom* geoms, TexGSBinning* bins, const TexGSImage* imgs, int32_t count,
                         void* stream) {
    if (int r = check_views(frames, count)) return r;
    if (!geoms || !bins || !imgs) return fail_msg("NULL argument");
    const CamConst c = make_cam(&frames[0]);
    const uint32_t T = (uint32_t)(c.tiles_x * c.tiles_y);
    for (int32_t v = 0; v < count; ++v) {
        const TexGSBinning& b = bins[v];
        if (!geoms[v].offsets || !geoms[v].rect || !geoms[v].tiles_touched || !geoms[v].scan_temp) return fail_msg("NULL buffer in a view's TexGSGeom");
        if (!b.ranges || !b.tile_order) return fail_msg("NULL ranges / tile_order in a view's TexGSBinning");
        if (b.num_rendered > 0) {
            if (!b.keys_unsorted || !b.keys_sorted || !b.point_list || !b.sort_temp) return fail_msg("NULL buffer in a view's TexGSBinning");
            if (b.sort_temp_bytes < sort_temp_bytes(b.num_rendered, T)) return fail_msg("sort_temp too small");
        }
        if ((imgs[v].tex_bin_count != nullptr) && frames[v].tex_res != frames[0].tex_res) return fail_msg("the views of a batch must have one tex_res");
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t st;
    const int nzw = 2 * (int)tex_bin_count(c.R);
    { ProfScope p(TEXGS_K_DUPLICATE, s); st = launch_bin_views(TEXGS_K_DUPLICATE, c, geoms, bins, imgs, count, nzw, s); }
    if (int r = launched("duplicate_with_keys (views)", st, s, frames[0].debug)) return r;
    { ProfScope p(TEXGS_K_SORT, s); st = launch_bin_views(TEXGS_K_SORT, c, geoms, bins, imgs, count, nzw, s); }
    if (int r = launched("tile sort (views)", st, s, frames[0].debug)) return r;
    { ProfScope p(TEXGS_K_RANGES, s); st = launch_bin_views(TEXGS_K_RANGES, c, geoms, bins, imgs, count, nzw, s); }
    return launched("tile_ranges (views)", st, s, frames[0].debug);
}

int texgs_render_forward_binned(const TexGSFrame* frame, const TexGSInputs* in, const TexGSGeom* geom, const TexGSBinning* bin,
                                TexGSImage* img, void* stream) {
    return render_forward_impl(frame, in, geom, bin, img, stream, true);
}

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
    snprintf(g_err, sizeof(g_err), "the fused MLP does not support this shape: %s, got %d", what, v);
    return -1;
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

// include/texgs_present.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_present_image(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return fail_msg("height and width must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("image too large: height * width must be below 2^31");
    return 0;
}

static int check_present_outputs(const uint8_t* u8, int32_t u8_channels, const float* hwc4, const float* chw) {
    if (!u8 && !hwc4 && !chw) return fail_msg("no output requested (out_u8, out_hwc4 and out_chw are all NULL)");
    if (u8) {
        if (u8_channels != 3 && u8_channels != 4) return fail_msg("u8_channels must be 3 or 4");
        if ((uintptr_t)u8 & (u8_channels == 4 ? 15 : 3)) return fail_msg("out_u8 must be 4-byte aligned with 3 channels, 16-byte aligned with 4");
    }
    if ((uintptr_t)hwc4 & 15) return fail_msg("out_hwc4 must be 16-byte aligned");
    if ((uintptr_t)chw & 3) return fail_msg("out_chw must be 4-byte aligned");
    return 0;
}

int texgs_present(const TexGSPresent* p, void* stream) {
    if (!p) return fail_msg("present descriptor is NULL");
    if (int r = check_present_image(p->height, p->width)) return r;
    if (!p->src) return fail_msg("NULL argument (src)");
    if (p->channels != 1 && p->channels != 3) return fail_msg("channels must be 1 or 3");
    if (p->flags & ~(TEXGS_PRESENT_AFFINE | TEXGS_PRESENT_COMPOSITE | TEXGS_PRESENT_SWAP_RB)) return fail_msg("unknown bit in flags");
    if ((p->flags & TEXGS_PRESENT_COMPOSITE) && !p->alpha) return fail_msg("composite mode needs alpha");
    if (int r = check_present_outputs(p->out_u8, p->u8_channels, p->out_hwc4, p->out_chw)) return r;
    if (((uintptr_t)p->src | (uintptr_t)p->alpha | (uintptr_t)p->background) & 3) return fail_msg("src, alpha and background must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("present", launch_present(p, s), s, false);
}

size_t texgs_depth_colour_temp_bytes(int32_t height, int32_t width) {
    return check_present_image(height, width) ? 0 : depth_colour_temp_bytes(height, width);
}

int texgs_depth_colour(const TexGSDepthColour* d, void* temp, size_t temp_bytes, void* stream) {
    if (!d) return fail_msg("depth descriptor is NULL");
    if (int r = check_present_image(d->height, d->width)) return r;
    if (!d->depth || !d->lut || !temp) return fail_msg("NULL argument (depth, lut or temp)");
    if (d->flags & ~TEXGS_PRESENT_SWAP_RB) return fail_msg("unknown bit in flags (the depth picture reads TEXGS_PRESENT_SWAP_RB only)");
    if (int r = check_present_outputs(d->out_u8, d->u8_channels, d->out_hwc4, d->out_chw)) return r;
    if (((uintptr_t)d->depth | (uintptr_t)d->mask | (uintptr_t)d->range | (uintptr_t)temp) & 3)
        return fail_msg("depth, mask, range and temp must be 4-byte aligned");
    if (temp_bytes < depth_colour_temp_bytes(d->height, d->width)) return fail_msg("temp is smaller than texgs_depth_colour_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("depth_colour", launch_depth_colour(d, temp, s), s, false);
}

int texgs_cube_cross(const TexGSCubeCross* c, void* stream) {
    if (!c) return fail_msg("cross descriptor is NULL");
    if (c->res < 1 || c->res > 7168) return fail_msg("res must be in [1,7168]");
    if (!c->texture || !c->out) return fail_msg("NULL argument (texture or out)");
    if (((uintptr_t)c->texture | (uintptr_t)c->out) & 3) return fail_msg("texture and out must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("cube_cross", launch_cube_cross(c, s), s, false);
}

// include/texgs_ingest.h: every argument is checked before the first launch, so a refused call has changed nothing
static int fail_fmt(const char* fmt, long long v, long long w = 0) {
    snprintf(g_err, sizeof(g_err), fmt, v, w);
    return -1;
}

// One axis in_size -> out_size: its ksize, or 0 with the cause in the error text
static int check_resize_axis(const char* what, int32_t in_size, int32_t out_size, int32_t filter) {
    if (filter != TEXGS_INGEST_BICUBIC && filter != TEXGS_INGEST_BILINEAR && filter != TEXGS_INGEST_BOX) {
        fail_fmt("unknown filter %lld (TEXGS_INGEST_BICUBIC, _BILINEAR or _BOX)", filter);
        return 0;
    }
    if (in_size < 1 || out_size < 1) {
        snprintf(g_err, sizeof(g_err), "%s: sizes must be positive, got %d -> %d", what, in_size, out_size);
        return 0;
    }
    if (in_size > TEXGS_INGEST_MAX_SIDE || out_size > TEXGS_INGEST_MAX_SIDE) {
        snprintf(g_err, sizeof(g_err), "%s: %d -> %d: an image side above %d is not supported", what, in_size, out_size, TEXGS_INGEST_MAX_SIDE);
        return 0;
    }
    const int k = ingest_ksize(in_size, out_size, filter);
    if (k > TEXGS_INGEST_MAX_KSIZE) {
        snprintf(g_err, sizeof(g_err), "%s: %d -> %d needs ksize %d taps per output, above the limit of %d", what, in_size, out_size, k,
                 TEXGS_INGEST_MAX_KSIZE);
        return 0;
    }
    return k;
}

static int check_resize_shape(int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, int32_t filter) {
    if (C == 4) return fail_msg("channels = 4 (RGBA) is not supported: Pillow premultiplies alpha before it resamples; composite first");
    if (C != 1 && C != 3) return fail_fmt("channels must be 1 or 3, got %lld", C);
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
        return fail_fmt("%lld x %lld: an image side above 16384 is not supported", height, width);
    if (!rgba || !out) return fail_msg("NULL argument (rgba or out)");
    if (((uintptr_t)rgba | (uintptr_t)out) & 3) return fail_msg("rgba and out must be 4-byte aligned");
    if (!(bg_r >= 0.0 && bg_r <= 1.0 && bg_g >= 0.0 && bg_g <= 1.0 && bg_b >= 0.0 && bg_b <= 1.0))
        return fail_msg("the background must lie in [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    return launched("rgba_composite", launch_rgba_composite(rgba, out, height, width, bg_r, bg_g, bg_b, s), s, false);
}

// include/texgs_surface.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_surface_image(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return fail_msg("image size must be positive");
    if (H > TEXGS_SURFACE_MAX_SIDE || W > TEXGS_SURFACE_MAX_SIDE) return fail_fmt("%lld x %lld: an image side above 16384 is not supported", H, W);
    if ((long long)H * W >= (1ll << 31)) return fail_msg("image too large: height * width must be below 2^31");
    return 0;
}

size_t texgs_surface_temp_bytes(int32_t height, int32_t width) {
    return check_surface_image(height, width) ? 0 : surface_temp_bytes(height, width);
}

int texgs_surface_points(const TexGSSurfacePoints* p, void* temp, size_t temp_bytes, void* stream) {
    if (!p) return fail_msg("surface descriptor is NULL");
    if (int r = check_surface_image(p->height, p->width)) return r;
    if (!p->depth || !p->alpha || !p->full_proj || !p->xyz || !p->count || !temp)
        return fail_msg("NULL argument (depth, alpha, full_proj, xyz, count or temp)");
    if (!(p->zfar == p->zfar) || !(p->znear == p->znear) || p->zfar == p->znear) return fail_msg("zfar and znear must be two different numbers");
    if (!(p->threshold == p->threshold)) return fail_msg("threshold is NaN");
    if ((long long)p->capacity < (long long)p->height * p->width)
        return fail_msg("capacity must be at least height * width (the count is not known before the launches)");
    if (((uintptr_t)p->depth | (uintptr_t)p->alpha | (uintptr_t)p->full_proj | (uintptr_t)p->xyz | (uintptr_t)p->alpha_sel | (uintptr_t)p->rank |
         (uintptr_t)p->count) & 3)
        return fail_msg("depth, alpha, full_proj, xyz, alpha_sel, rank and count must be 4-byte aligned");
    if (((uintptr_t)p->index | (uintptr_t)temp) & 7) return fail_msg("index and temp must be 8-byte aligned");
    if (temp_bytes < surface_temp_bytes(p->height, p->width)) return fail_msg("temp is smaller than texgs_surface_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("surface_points", launch_surface_points(p, temp, s), s, false);
}

int texgs_surface_compose(const TexGSSurfaceCompose* c, void* stream) {
    if (!c) return fail_msg("compose descriptor is NULL");
    if (int r = check_surface_image(c->height, c->width)) return r;
    if (c->rows < 0) return fail_msg("rows < 0");
    if (!c->rank || !c->alpha || !c->out || (c->rows > 0 && !c->values)) return fail_msg("NULL argument (values, rank, alpha or out)");
    if (((uintptr_t)c->values | (uintptr_t)c->rank | (uintptr_t)c->alpha | (uintptr_t)c->background | (uintptr_t)c->out) & 3)
        return fail_msg("values, rank, alpha, background and out must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("surface_compose", launch_surface_compose(c, s), s, false);
}

// include/texgs_lpips.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_lpips_precision(int32_t precision) {
    if (precision == TEXGS_LPIPS_FP32) return 0;
    if (precision == TEXGS_LPIPS_BF16X3) return fail_msg("precision TEXGS_LPIPS_BF16X3 is not built into this library: use TEXGS_LPIPS_FP32");
    snprintf(g_err, sizeof(g_err), "unknown precision %d (TEXGS_LPIPS_FP32 is 0)", (int)precision);
    return -1;
}

static int check_conv_channels(int32_t Cin, int32_t Cout, int32_t precision) {
    if (int r = check_lpips_precision(precision)) return r;
    if (Cin < 1 || Cin > TEXGS_CONV_MAX_CHANNELS) { snprintf(g_err, sizeof(g_err), "Cin must be in [1,512], got %d", (int)Cin); return -1; }
    if (Cout < 16 || Cout > TEXGS_CONV_MAX_CHANNELS || Cout % 16) {
        snprintf(g_err, sizeof(g_err), "Cout must be a multiple of 16 in [16,512], got %d", (int)Cout);
        return -1;
    }
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

// the strides of a [B, Cn, h, w] view in floats: all zero (dense), or no two elements on one address and B img below 2^62
static int check_conv_strides(const char* name, int64_t row, int64_t chan, int64_t img, int64_t B, int64_t Cn, int64_t h, int64_t w) {
    if (row == 0 && chan == 0 && img == 0) return 0;
    if (row < w || chan < 0 || img < 0 || chan / h < row || img / Cn < chan || img > (1ll << 62) / B) {
        snprintf(g_err, sizeof(g_err), "%s_row, %s_chan, %s_img must be all 0 (dense) or row >= width, chan >= rows x row, img >= channels x chan, "
                 "B x img <= 2^62; got %lld, %lld, %lld", name, name, name, (long long)row, (long long)chan, (long long)img);
        return -1;
    }
    return 0;
}

int texgs_conv3x3(const TexGSConv3x3* d, void* stream) {
    if (!d) return fail_msg("conv descriptor is NULL");
    if (int r = check_conv_channels(d->Cin, d->Cout, d->precision)) return r;
    if ((d->relu != 0 && d->relu != 1) || (d->pool_in != 0 && d->pool_in != 1)) return fail_msg("relu and pool_in must be 0 or 1");
    if (d->B < 1 || d->B > TEXGS_CONV_MAX_BATCH) { snprintf(g_err, sizeof(g_err), "B must be in [1,65535], got %d", (int)d->B); return -1; }
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

static int check_lpips_head_size(int32_t P, int32_t h, int32_t w) {
    if (P < 1 || P > 65535) { snprintf(g_err, sizeof(g_err), "P must be in [1,65535], got %d", (int)P); return -1; }
    if (h < 1 || w < 1) return fail_msg("h and w must be at least 1");
    if ((int64_t)h * w >= (1ll << 31)) return fail_msg("map too large: h w must be below 2^31");
    return 0;
}

size_t texgs_lpips_head_temp_bytes(int32_t P, int32_t h, int32_t w) { return check_lpips_head_size(P, h, w) ? 0 : lpips_head_temp_bytes(P, h, w); }

int texgs_lpips_head(const TexGSLpipsHead* d, void* stream) {
    if (!d) return fail_msg("head descriptor is NULL");
    if (int r = check_lpips_head_size(d->P, d->h, d->w)) return r;
    if (d->C < 1 || d->C > TEXGS_CONV_MAX_CHANNELS) { snprintf(g_err, sizeof(g_err), "C must be in [1,512], got %d", (int)d->C); return -1; }
    if (d->layer < 0 || d->layer >= TEXGS_LPIPS_LAYERS) { snprintf(g_err, sizeof(g_err), "layer must be in [0,4], got %d", (int)d->layer); return -1; }
    if (!d->f || !d->lin || !d->out || !d->temp) return fail_msg("NULL argument (f, lin, out or temp)");
    if (((uintptr_t)d->f | (uintptr_t)d->lin) & 3) return fail_msg("f and lin must be 4-byte aligned");
    if (((uintptr_t)d->out | (uintptr_t)d->temp) & 7) return fail_msg("out and temp must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("lpips_head", launch_lpips_head(d, s), s, false);
}

// include/texgs_lpips_grad.h
int texgs_lpips_head_backward(const TexGSLpipsHeadBackward* d, void* stream) {
    if (!d) return fail_msg("head backward descriptor is NULL");
    if (int r = check_lpips_head_size(d->P, d->h, d->w)) return r;
    if (d->C < 1 || d->C > TEXGS_CONV_MAX_CHANNELS) { snprintf(g_err, sizeof(g_err), "C must be in [1,512], got %d", (int)d->C); return -1; }
    if (d->wrt < 1 || d->wrt > (TEXGS_LPIPS_WRT_FIRST | TEXGS_LPIPS_WRT_PARTNER)) {
        snprintf(g_err, sizeof(g_err), "wrt must be 1 (first images), 2 (partners) or 3 (both), got %d", (int)d->wrt);
        return -1;
    }
    if (d->g_next && (d->h < 2 || d->w < 2)) return fail_msg("g_next needs h and w of at least 2: the pooled map would be empty");
    const int64_t Bg = d->wrt == 3 ? 2 * (int64_t)d->P : d->P;
    if (int r = check_conv_strides("g", d->g_row, d->g_chan, d->g_img, Bg, d->C, d->h, d->w)) return r;
    if (!d->f || !d->lin || !d->gbar || !d->G) return fail_msg("NULL argument (f, lin, gbar or G)");
    if (((uintptr_t)d->f | (uintptr_t)d->lin | (uintptr_t)d->gbar | (uintptr_t)d->g_next | (uintptr_t)d->G) & 3)
        return fail_msg("f, lin, gbar, g_next and G must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("lpips_head_backward", launch_lpips_head_backward(d, s), s, false);
}

int texgs_lpips_gate(float* G, const float* y, int64_t n, void* stream) {
    if (n < 1 || n >= (1ll << 40)) { snprintf(g_err, sizeof(g_err), "n must be in [1,2^40), got %lld", (long long)n); return -1; }
    if (!G || !y) return fail_msg("NULL argument (G or y)");
    if (((uintptr_t)G | (uintptr_t)y) & 15) return fail_msg("G and y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("lpips_gate", launch_lpips_gate(G, y, n, s), s, false);
}

// include/texgs_params.h: every argument is checked before the first launch, so a refused call has changed nothing
static int check_params_epsilon(float e) {
    if (!(e > 0.0f && e < 0.5f)) return fail_msg("epsilon must lie in (0, 0.5)");
    return 0;
}

static int check_params_modifier(float m) {
    if (!(m > 0.0f) || m - m != 0.0f) return fail_msg("scale_modifier must be finite and positive");
    return 0;
}

size_t texgs_params_temp_bytes(int32_t n) { return n <= 0 ? 0 : params_temp_bytes(n); }

int texgs_params_activate(const TexGSParamsActivate* a, void* temp, size_t temp_bytes, void* stream) {
    if (!a) return fail_msg("activate descriptor is NULL");
    if (a->n < 0) return fail_msg("n < 0");
    if (a->reg) {
        if (int r = check_params_epsilon(a->epsilon)) return r;
        if (a->n == 0) return fail_msg("reg with n = 0: a mean over nothing");
    }
    if (a->n == 0) return 0;
    if (!a->scales && !a->rotations && !a->opacities && !a->reg)
        return fail_msg("no output requested (scales, rotations, opacities and reg are all NULL)");
    if ((a->scales && !a->scaling) || (a->rotations && !a->rotation) || ((a->opacities || a->reg) && !a->opacity))
        return fail_msg("NULL argument (scaling, rotation or opacity: the input of a requested output)");
    if (a->reg && !temp) return fail_msg("NULL argument (temp, needed with reg)");
    if (((uintptr_t)a->scaling | (uintptr_t)a->opacity | (uintptr_t)a->scales | (uintptr_t)a->opacities | (uintptr_t)a->reg) & 3)
        return fail_msg("scaling, opacity, scales, opacities and reg must be 4-byte aligned");
    if (((uintptr_t)a->rotation | (uintptr_t)a->rotations) & 15) return fail_msg("rotation and rotations must be 16-byte aligned");
    if (a->reg && ((uintptr_t)temp & 7)) return fail_msg("temp must be 8-byte aligned");
    if (a->reg && temp_bytes < params_temp_bytes(a->n)) return fail_msg("temp is smaller than texgs_params_temp_bytes");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_activate", launch_params_activate(a, temp, s), s, false);
}

int texgs_params_activate_backward(const TexGSParamsActivateGrad* g, void* stream) {
    if (!g) return fail_msg("activate backward descriptor is NULL");
    if (g->n < 0) return fail_msg("n < 0");
    if (g->g_reg)
        if (int r = check_params_epsilon(g->epsilon)) return r;
    if (g->n == 0) return 0;
    if (!g->d_scaling && !g->d_rotation && !g->d_opacity)
        return fail_msg("no output requested (d_scaling, d_rotation and d_opacity are all NULL)");
    if ((g->d_scaling && g->g_scales && !g->scales) || (g->d_rotation && g->g_rotations && !g->rotation) ||
        (g->d_opacity && (g->g_opacities || g->g_reg) && !g->opacities))
        return fail_msg("NULL argument (scales, rotation or opacities: read for a requested output with an upstream gradient)");
    if (((uintptr_t)g->scales | (uintptr_t)g->opacities | (uintptr_t)g->g_scales | (uintptr_t)g->g_opacities | (uintptr_t)g->g_reg |
         (uintptr_t)g->d_scaling | (uintptr_t)g->d_opacity) & 3)
        return fail_msg("scales, opacities, g_scales, g_opacities, g_reg, d_scaling and d_opacity must be 4-byte aligned");
    if (((uintptr_t)g->rotation | (uintptr_t)g->g_rotations | (uintptr_t)g->d_rotation) & 15)
        return fail_msg("rotation, g_rotations and d_rotation must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_activate_backward", launch_params_activate_backward(g, s), s, false);
}

int texgs_params_covariance(const TexGSParamsCovariance* c, void* stream) {
    if (!c) return fail_msg("covariance descriptor is NULL");
    if (c->n < 0) return fail_msg("n < 0");
    if (int r = check_params_modifier(c->scale_modifier)) return r;
    if (c->n == 0) return 0;
    if (!c->scaling || !c->rotation || !c->cov) return fail_msg("NULL argument (scaling, rotation or cov)");
    if (((uintptr_t)c->scaling | (uintptr_t)c->cov) & 3) return fail_msg("scaling and cov must be 4-byte aligned");
    if ((uintptr_t)c->rotation & 15) return fail_msg("rotation must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_covariance", launch_params_covariance(c, s), s, false);
}

int texgs_params_covariance_backward(const TexGSParamsCovarianceGrad* c, void* stream) {
    if (!c) return fail_msg("covariance backward descriptor is NULL");
    if (c->n < 0) return fail_msg("n < 0");
    if (int r = check_params_modifier(c->scale_modifier)) return r;
    if (c->n == 0) return 0;
    if (!c->d_scaling && !c->d_rotation) return fail_msg("no output requested (d_scaling and d_rotation are both NULL)");
    if (!c->scaling || !c->rotation) return fail_msg("NULL argument (scaling or rotation)");
    if (((uintptr_t)c->scaling | (uintptr_t)c->g_cov | (uintptr_t)c->d_scaling) & 3) return fail_msg("scaling, g_cov and d_scaling must be 4-byte aligned");
    if (((uintptr_t)c->rotation | (uintptr_t)c->d_rotation) & 15) return fail_msg("rotation and d_rotation must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return launched("params_covariance_backward", launch_params_covariance_backward(c, s), s, false);
}

// include/texgs_retexture.h: every argument is checked before the launch, so a refused call has changed nothing
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

static int check_retexture(const void* src, size_t src_bytes, const float* old_tex, float* out_tex, int32_t R, int32_t mode) {
    if (R < 1 || R > TEXGS_RETEX_MAX_RES) return fail_msg("R must be in [1,7168]");
    if (mode < -1 || mode > 3) return fail_msg("mode must be -1, 0, 1, 2 or 3");
    if (!src) return fail_msg("NULL argument (src)");
    if (!out_tex) return fail_msg("NULL argument (out_tex)");
    if (!old_tex && mode != -1) return fail_msg("NULL argument (old_tex): only mode -1 does without the old texture");
    if (((uintptr_t)old_tex | (uintptr_t)out_tex) & 3) return fail_msg("old_tex and out_tex must be 4-byte aligned");
    const size_t tex_bytes = 6 * (size_t)R * (size_t)R * 3 * sizeof(float);
    if (old_tex && old_tex != out_tex && ranges_overlap(old_tex, tex_bytes, out_tex, tex_bytes))
        return fail_msg("out_tex overlaps old_tex without being equal to it (in place means the same pointer)");
    if (ranges_overlap(src, src_bytes, out_tex, tex_bytes)) return fail_msg("out_tex overlaps src");
    return 0;
}

int texgs_retexture_cross(const TexGSRetexCross* c, void* stream) {
    if (!c) return fail_msg("retexture cross descriptor is NULL");
    if (c->r < 1 || c->r > TEXGS_RETEX_MAX_SRC) return fail_msg("r must be in [1,16384]");
    if (c->order != TEXGS_RETEX_RGB && c->order != TEXGS_RETEX_BGR) return fail_msg("order must be 0 (rgb) or 1 (bgr)");
    if (int rc = check_retexture(c->src, 36 * (size_t)c->r * (size_t)c->r, c->old_tex, c->out_tex, c->R, c->mode)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return launched("retexture_cross", launch_retexture_cross(c, s), s, false);
}

int texgs_retexture_latlong(const TexGSRetexLatLong* l, void* stream) {
    if (!l) return fail_msg("retexture latlong descriptor is NULL");
    if (l->h < 1 || l->h > TEXGS_RETEX_MAX_SRC || l->w < 1 || l->w > TEXGS_RETEX_MAX_SRC) return fail_msg("h and w must be in [1,16384]");
    if (l->src_u8 != 0 && l->src_u8 != 1) return fail_msg("src_u8 must be 0 or 1");
    if (!l->src_u8 && ((uintptr_t)l->src & 3)) return fail_msg("a float src must be 4-byte aligned");
    const size_t src_bytes = 3 * (size_t)l->h * (size_t)l->w * (l->src_u8 ? 1 : sizeof(float));
    if (int rc = check_retexture(l->src, src_bytes, l->old_tex, l->out_tex, l->R, l->mode)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return launched("retexture_latlong", launch_retexture_latlong(l, s), s, false);
}

// include/texgs_shcolor.h: every argument is checked before the launch, so a refused call has changed nothing
static int check_sh_colors(int32_t n, int32_t coeffs, int32_t degree, int32_t layout, int32_t mode, int32_t count, const void* sh,
                           const void* sh_dc, const void* sh_rest, const void* views) {
    if (degree < 0 || degree > TEXGS_SH_COLORS_MAX_DEGREE) return fail_msg("degree must be in [0,4]");
    if (coeffs != 1 && coeffs != 4 && coeffs != 9 && coeffs != 16 && coeffs != 25) return fail_msg("coeffs must be 1, 4, 9, 16 or 25");
    if ((degree + 1) * (degree + 1) > coeffs) return fail_msg("(degree + 1)^2 exceeds coeffs");
    if (n < 0) return fail_msg("n < 0");
    if ((int64_t)n * coeffs * 3 >= (1ll << 31)) return fail_msg("n * coeffs * 3 must be below 2^31");
    if (layout != TEXGS_SH_LAYOUT_KC && layout != TEXGS_SH_LAYOUT_CK) return fail_msg("layout must be 0 ([n,coeffs,3]) or 1 ([n,3,coeffs])");
    if (mode != TEXGS_SH_COLORS && mode != TEXGS_SH_EVAL) return fail_msg("mode must be 0 (colours) or 1 (eval_sh)");
    if (count < 1) return fail_msg("count < 1: at least one view");
    if (count > TEXGS_SH_COLORS_MAX_VIEWS) return fail_msg("count exceeds TEXGS_SH_COLORS_MAX_VIEWS: several calls");
    if (mode == TEXGS_SH_EVAL && count != 1) return fail_msg("mode eval_sh takes exactly one view");
    if (!views) return fail_msg("NULL argument (views)");
    if (sh && (sh_dc || sh_rest)) return fail_msg("both sh and the pair (sh_dc, sh_rest) are set");
    if (!sh && layout != TEXGS_SH_LAYOUT_KC) return fail_msg("the pair (sh_dc, sh_rest) has layout 0 only");
    if (n == 0) return 0;
    if (!sh && !sh_dc) return fail_msg("NULL argument (sh, or sh_dc of the pair)");
    if (!sh && !sh_rest && degree > 0) return fail_msg("NULL argument (sh_rest: read at degree >= 1)");
    if (((uintptr_t)sh | (uintptr_t)sh_dc | (uintptr_t)sh_rest) & 3) return fail_msg("sh, sh_dc and sh_rest must be 4-byte aligned");
    return 0;
}

int texgs_sh_colors_forward(const TexGSShColors* c, const TexGSShColorView* views, int32_t count, void* stream) {
    if (!c) return fail_msg("sh colours descriptor is NULL");
    if (int r = check_sh_colors(c->n, c->coeffs, c->degree, c->layout, c->mode, count, c->sh, c->sh_dc, c->sh_rest, views)) return r;
    if (c->n == 0) return 0;
    if (c->degree > 0 && !c->xyz) return fail_msg("NULL argument (xyz: read at degree >= 1)");
    if ((uintptr_t)c->xyz & 3) return fail_msg("xyz must be 4-byte aligned");
    for (int v = 0; v < count; ++v) {
        if (!views[v].colors) return fail_msg("NULL argument (a view's colors)");
        if (c->degree > 0 && c->mode == TEXGS_SH_COLORS && !views[v].campos) return fail_msg("NULL argument (a view's campos: read at degree >= 1)");
        if (((uintptr_t)views[v].colors | (uintptr_t)views[v].campos) & 3) return fail_msg("a view's campos and colors must be 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    return launched("sh_colors_forward", launch_sh_colors(c, views, count, s), s, false);
}

int texgs_sh_colors_backward(const TexGSShColorsGrad* g, const TexGSShColorGradView* views, int32_t count, void* stream) {
    if (!g) return fail_msg("sh colours backward descriptor is NULL");
    if (int r = check_sh_colors(g->n, g->coeffs, g->degree, g->layout, g->mode, count, g->sh, g->sh_dc, g->sh_rest, views)) return r;
    if (g->accumulate != 0 && g->accumulate != 1) return fail_msg("accumulate must be 0 or 1");
    if (g->n == 0) return 0;
    if (!g->d_sh && !g->d_sh_dc && !g->d_sh_rest && !g->d_xyz)
        return fail_msg("no output requested (d_sh, d_sh_dc, d_sh_rest and d_xyz are all NULL)");
    if (g->d_sh && !g->sh) return fail_msg("d_sh belongs to sh, which is NULL");
    if ((g->d_sh_dc || g->d_sh_rest) && g->sh) return fail_msg("d_sh_dc and d_sh_rest belong to the pair, but sh is set");
    if (g->degree > 0 && !g->xyz) return fail_msg("NULL argument (xyz: read at degree >= 1)");
    if (((uintptr_t)g->xyz | (uintptr_t)g->d_sh | (uintptr_t)g->d_sh_dc | (uintptr_t)g->d_sh_rest | (uintptr_t)g->d_xyz) & 3)
        return fail_msg("xyz, d_sh, d_sh_dc, d_sh_rest and d_xyz must be 4-byte aligned");
    for (int v = 0; v < count; ++v) {
        if (!views[v].g_colors) return fail_msg("NULL argument (a view's g_colors)");
        if (g->degree > 0 && g->mode == TEXGS_SH_COLORS && !views[v].campos) return fail_msg("NULL argument (a view's campos: read at degree >= 1)");
        if (((uintptr_t)views[v].g_colors | (uintptr_t)views[v].campos) & 3) return fail_msg("a view's campos and g_colors must be 4-byte aligned");
    }
    hipStream_t s = (hipStream_t)stream;
    return launched("sh_colors_backward", launch_sh_colors_backward(g, views, count, s), s, false);
}

int texgs_selftest_waveops(const float* seed128, float* out576, void* stream) {
    if (!seed128 || !out576) return fail_msg("NULL argument");
    return launched("selftest_waveops", launch_selftest_waveops(seed128, out576, (hipStream_t)stream), (hipStream_t)stream, false);
}

int texgs_mark_visible(const TexGSFrame* frame, const float* means3D, uint8_t* visible, void* stream) {
    if (int r = validate_frame(frame)) return r;
    if (!means3D || !visible) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("mark_visible", launch_mark_visible(frame, means3D, visible, s), s, frame->debug);
}

}  // extern "C"
