// C-ABI entry points of the rasterizer (K1-K8, the batched front end, the SH flush: include/texgs.h and
// include/texgs_multiview.h) and the error plumbing of every unit (abi_support.h).  Each other stage defines its entry
// points in its own unit, below its launchers.  No C++ types or exceptions cross this boundary: int return codes + a
// thread-local error string.
#include "common.h"
#include "abi_support.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

namespace {

thread_local char g_err[512] = "";     // the one error string: a refusal raised in any unit lands here

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

// ---- abi_support.h ----
int fail(const char* where, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return (int)e ? (int)e : -1;
}

int fail_msg(const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return -1;
}

int failf(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return -1;
}

// (lineage `debug` semantics of the stream sync: render/uv_tex_render.py:37)
int launched(const char* where, hipError_t st, hipStream_t s, bool debug) {
    if (st == hipSuccess && debug) st = hipStreamSynchronize(s);
    return st == hipSuccess ? 0 : fail(where, st);
}

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
        if (v.sh_coeffs != K)
            return failf("K does not match: view %d wrote its residue with K = %d, the flush has K = %d", (int)k, (int)v.sh_coeffs, (int)K);
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

int texgs_mark_visible(const TexGSFrame* frame, const float* means3D, uint8_t* visible, void* stream) {
    if (int r = validate_frame(frame)) return r;
    if (!means3D || !visible) return fail_msg("NULL argument");
    hipStream_t s = (hipStream_t)stream;
    return launched("mark_visible", launch_mark_visible(frame, means3D, visible, s), s, frame->debug);
}

}  // extern "C"
