"""ctypes binding of libtexgs.so (C ABI in include/texgs.h).  Fails loudly when the HIP library is missing:
there is no CPU / eager fallback for the product path."""
import contextlib
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TEXGS_LIB") or os.path.join(os.path.dirname(_HERE), "libtexgs.so")   # TEXGS_LIB: experiment builds only

ABI_VERSION = 19
TILE = 16
REC_TEST_FLOATS = 8
REC_SHADE_FLOATS = 20
TEXBIN_RECORD_FLOATS = 4        # 16-byte texture-gradient records (TexGSGrads.tex_bins)
RESV_WORDS = 192         # per 8x8 pixel block: 64 reservation entries x {bin, offset, count} (TexGSImage.tex_bin_resv)
ACC_FLOATS = 32
WANT_TEXTURE, WANT_GAUSSIANS, WANT_ALL = 1, 2, 3

_fp = C.c_void_p  # device pointers travel as integers


class Frame(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float),
                ("tanfovy", C.c_float), ("scale_modifier", C.c_float), ("sh_degree", C.c_int32),
                ("sh_coeffs", C.c_int32), ("tex_res", C.c_int32), ("num_gaussians", C.c_int32),
                ("debug", C.c_int32), ("bg", _fp), ("viewmatrix", _fp), ("projmatrix", _fp), ("campos", _fp)]


class Inputs(C.Structure):
    _fields_ = [("means3D", _fp), ("shs", _fp), ("opacities", _fp), ("scales", _fp), ("rotations", _fp),
                ("uvs", _fp), ("gradient_uvs", _fp), ("texture", _fp), ("color_offset", _fp), ("cov3D_precomp", _fp)]


class Geom(C.Structure):
    _fields_ = [("rec_test", _fp), ("rec_shade", _fp), ("depth", _fp), ("radii", _fp), ("rect", _fp), ("tiles_touched", _fp),
                ("offsets", _fp), ("scan_temp", _fp), ("scan_temp_bytes", C.c_size_t)]


class Binning(C.Structure):
    _fields_ = [("num_rendered", C.c_uint32), ("keys_unsorted", _fp), ("keys_sorted", _fp), ("point_list", _fp),
                ("ranges", _fp), ("tile_order", _fp), ("sort_temp", _fp), ("sort_temp_bytes", C.c_size_t)]


class Image(C.Structure):
    _fields_ = [("out_color", _fp), ("out_depth", _fp), ("out_norm", _fp), ("out_alpha", _fp),
                ("final_T", _fp), ("n_contrib", _fp), ("tex_bin_count", _fp),
                ("survivors", _fp), ("surv_qmask", _fp), ("surv_count", _fp), ("tex_bin_resv", _fp)]


class Grads(C.Structure):
    _fields_ = [("dL_dcolor", _fp), ("dL_ddepth", _fp), ("dL_dnorm", _fp), ("dL_dalpha", _fp), ("acc", _fp),
                ("dL_dmeans3D", _fp), ("dL_dmeans2D", _fp), ("dL_dshs", _fp), ("dL_dopacities", _fp),
                ("dL_dscales", _fp), ("dL_drotations", _fp), ("dL_duvs", _fp), ("dL_dtexture", _fp),
                ("dL_dcolor_offset", _fp), ("dL_dcov3D", _fp), ("want", C.c_uint32), ("tex_bins", _fp), ("tex_bin_cursor", _fp), ("tex_bin_base", _fp),
                ("tex_rec_cap", C.c_uint32),
                ("accumulate", C.c_int32), ("dL_dvd_residue", _fp)]


class UVNetStruct(C.Structure):
    _fields_ = [(n, _fp) for n in ("W1", "b1", "W2", "b2", "emb", "W3", "b3", "W4", "b4", "W5", "b5", "xyz_offset", "xyz_scale")] \
        + [("hidden", C.c_int32)]


class HashGridStruct(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("n_features", C.c_int32), ("log2_hashmap_size", C.c_int32), ("base_resolution", C.c_float),
                ("per_level_scale", C.c_float)]


HASHGRID_MAX_LEVELS = 16
HASHGRID_FEATURES = 4


class UVNetGradStruct(C.Structure):
    _fields_ = [(n, _fp) for n in ("dW1", "db1", "dW2", "db2", "dW3", "db3", "dW4", "db4", "dW5", "db5")]


DENSITY_KEEP, DENSITY_CLONE, DENSITY_CLONE_KEPT, DENSITY_SPLIT, DENSITY_CHILD = 1, 2, 4, 8, 16      # TEXGS_DENSITY_* action bits
DENSITY_ROW = {"copy": 0, "moment": 1, "scaling": 2, "xyz": 3}                                      # TEXGS_DENSITY_ROW_*
DENSITY_MAX_ROWS = 24
METRICS_ROW = 16         # f64 slots of one view's row (TEXGS_METRICS_*): 0 sum|d|, 1-3 sum d^2, 4-6 sum S, 7/8 MAE num/den, 9 HW, 10 cropped


class DensityPlanStruct(C.Structure):
    _fields_ = [("accum", _fp), ("denom", _fp), ("scaling", _fp), ("opacity", _fp), ("n", C.c_int32), ("max_grad", C.c_float),
                ("min_opacity", C.c_float), ("dense_scale", C.c_float), ("big_scale", C.c_float), ("densify", C.c_int32),
                ("use_big", C.c_int32)]


class DensityRowStruct(C.Structure):
    _fields_ = [("src", _fp), ("dst", _fp), ("width", C.c_int32), ("kind", C.c_int32)]


class DensityMoveStruct(C.Structure):
    _fields_ = [("row", DensityRowStruct * DENSITY_MAX_ROWS), ("rows", C.c_int32), ("n", C.c_int32), ("action", _fp), ("rank", _fp),
                ("n_kept", C.c_int32), ("n_clone", C.c_int32), ("n_split", C.c_int32), ("n_child", C.c_int32), ("scaling", _fp),
                ("rotation", _fp), ("noise", _fp)]


UV_PRECISION = {"fp32": 0, "bf16x3": 1, "mixed": 2}          # TEXGS_UV_FP32 / _BF16X3 / _MIXED


_P = C.POINTER
_i32, _u32, _f32, _size, _vp = C.c_int32, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p
_frame5 = [_P(Frame), _P(Inputs), _P(Geom), _P(Binning), _P(Image)]
# The C ABI of include/texgs.h, stated once: name -> (restype, argtypes), in the header's order (tests/test_abi.py compares every entry
# with the header's prototype through tests/abi_check.py, as each stage's test does for the stage's own table).  load() applies it;
# EXPORTS is its key list.
SIGNATURES = {
    "texgs_abi_version": (C.c_int, []),
    "texgs_build_id": (C.c_char_p, []),
    "texgs_last_error": (C.c_char_p, []),
    "texgs_scan_temp_bytes": (_size, [_i32]),
    "texgs_sort_temp_bytes": (_size, [_u32, _u32]),
    "texgs_tex_bin_count": (_size, [_i32]),
    "texgs_preprocess_forward": (C.c_int, [_P(Frame), _P(Inputs), _P(Geom), _vp]),
    "texgs_num_rendered_words": (_size, [_i32]),
    "texgs_num_rendered_begin": (C.c_int, [_P(Geom), _i32, _vp, _size, _i32, _vp]),
    "texgs_num_rendered_reduce": (C.c_int, [_vp, _i32, _P(_u32), _P(C.c_uint64)]),
    "texgs_depth_sort_scan": (C.c_int, [_P(Geom), _i32, _vp]),
    "texgs_bin_sort_render_forward": (C.c_int, _frame5 + [_vp]),
    "texgs_render_forward": (C.c_int, _frame5 + [_vp]),
    "texgs_backward": (C.c_int, _frame5 + [_P(Grads), _vp]),
    "texgs_backward_render": (C.c_int, _frame5 + [_P(Grads), _vp]),
    "texgs_backward_preprocess": (C.c_int, [_P(Frame), _P(Inputs), _P(Geom), _P(Grads), _vp]),
    "texgs_profile_enable": (C.c_int, [C.c_int]),
    "texgs_profile_select": (C.c_int, [_u32]),
    "texgs_profile_read": (C.c_int, [_P(_f32), _P(_u32)]),
    "texgs_rgb_alpha_loss": (C.c_int, [_vp] * 4 + [_i32, _i32, _f32, _f32] + [_vp] * 5),
    "texgs_geom_losses": (C.c_int, [_vp] * 6 + [_i32, _i32, _f32, _f32, _f32, _f32] + [_vp] * 4),
    "texgs_norm_from_depth": (C.c_int, [_vp, _vp, _f32, _f32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "texgs_uv_packed_bytes": (_size, [_i32]),
    "texgs_uv_pack": (C.c_int, [_P(UVNetStruct), _i32, _vp, _vp]),
    "texgs_uv_taylor_packed": (C.c_int, [_P(UVNetStruct), _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "texgs_uv_backward_temp_bytes": (_size, [_i32]),
    "texgs_uv_backward": (C.c_int, [_P(UVNetStruct), _i32, _vp, _vp, _i32, _P(UVNetGradStruct), _vp, _vp]),
    "texgs_hashgrid_levels": (C.c_int, [_P(HashGridStruct), _vp, _vp, _vp, _vp, _P(_u32)]),
    "texgs_hashgrid_forward": (C.c_int, [_P(HashGridStruct), _vp, _vp, _i32, _vp, _vp]),
    "texgs_hashgrid_backward_temp_bytes": (_size, [_P(HashGridStruct), _i32]),
    "texgs_hashgrid_backward": (C.c_int, [_P(HashGridStruct), _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "texgs_chamfer_nn_temp_bytes": (_size, [_i32]),
    "texgs_chamfer_nn": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "texgs_knn3_temp_bytes": (_size, [_i32]),
    "texgs_knn3_mean_dist2": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    "texgs_fps_temp_bytes": (_size, [_i32, _i32]),
    "texgs_farthest_points": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "texgs_cube_sample": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "texgs_cube_latlong": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "texgs_cube_sample_backward": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "texgs_cube_sample_nearest_backward": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "texgs_density_stats": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "texgs_density_plan_temp_bytes": (_size, [_i32]),
    "texgs_density_plan": (C.c_int, [_P(DensityPlanStruct), _vp, _vp, _vp, _vp, _vp]),
    "texgs_density_move": (C.c_int, [_P(DensityMoveStruct), _vp]),
    "texgs_eval_metrics_temp_bytes": (_size, [_i32, _i32]),
    "texgs_eval_metrics": (C.c_int, [_vp] * 5 + [_i32, _i32, _i32, _vp, _vp, _vp]),
    "texgs_selftest_waveops": (C.c_int, [_vp, _vp, _vp]),
    "texgs_mark_visible": (C.c_int, [_P(Frame), _vp, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)
KERNEL_NAMES = ["preprocess_fwd", "scan", "duplicate", "sort", "ranges", "render_fwd", "render_bwd", "preprocess_bwd",
                "texgrad_reduce"]

_lib = None
_bound = {}         # id(table) -> table, for every table that bind() has applied (holding the table keeps its id from being reused)


def _apply(lib, signatures):
    """Set restype / argtypes of every entry of a {name: (restype, argtypes)} table on `lib`; every name that `lib` lacks is reported"""
    missing = [n for n in signatures if not hasattr(lib, n)]
    if missing:         # a library from before an additive change of the ABI (the version number stays): same advice as a stale version
        raise RuntimeError(f"libtexgs.so at {LIB_PATH} does not export {', '.join(missing)}; rebuild it with "
                           "`python texture-gs_amd/build.py`")
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def bind(signatures):
    """The loaded library with a stage's own table applied: {name: (restype, argtypes)}, stated in the stage's module beside its struct
    mirrors (tests/abi_check.py compares it with the stage's header).  The table object is remembered, so every later call is one
    lookup."""
    if id(signatures) not in _bound:
        _apply(load(), signatures)
        _bound[id(signatures)] = signatures
    return _lib


def load():
    """Load libtexgs.so once.  Raises RuntimeError (never falls back) if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libtexgs.so not found at {LIB_PATH}: build it with `python texture-gs_amd/build.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the rasterizer.")
    lib = C.CDLL(LIB_PATH)
    _apply(lib, SIGNATURES)
    v = lib.texgs_abi_version()
    if v != ABI_VERSION:
        # (no bypass in the shipped loader -- the struct layouts differ between versions; experiment scripts that A/B an
        #  older build must run it under that build's own host layer)
        raise RuntimeError(f"libtexgs.so ABI version {v} != expected {ABI_VERSION}; rebuild it")
    global BUILD_ID
    BUILD_ID = lib.texgs_build_id().decode()
    if not os.environ.get("TEXGS_LIB"):          # the product library must be built from THIS tree's sources (experiment builds: any)
        want = tree_build_id()
        if want is not None and BUILD_ID != want:
            raise RuntimeError(f"libtexgs.so was built from other sources (build id {BUILD_ID}, this tree is {want}); "
                               "rebuild it with `python texture-gs_amd/build.py`")
    _lib = lib
    return lib


BUILD_ID = None


def tree_build_id():
    """The build id of the sources in this tree (texture-gs_amd/build.py build_id()); None if the build script is not there."""
    import importlib.util
    path = os.path.join(os.path.dirname(_HERE), "build.py")
    if not os.path.exists(path):
        return None
    spec = importlib.util.spec_from_file_location("texgs_build_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_id()


def check(rc, what):
    if rc != 0:
        msg = load().texgs_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def call(fn, *args):
    """Run one int-returning entry point of the library (`call(lib.texgs_x, ...)`); a non-zero code raises with the function's name."""
    rc = fn(*args)
    if rc != 0:         # (tested here, not only in check: the per-view path makes a dozen of these calls)
        check(rc, fn.__name__)


def ptr(t):
    """Device pointer of an optional tensor (None travels as NULL)."""
    return None if t is None else t.data_ptr()


@contextlib.contextmanager
def on(device):
    """Make `device` current and yield the raw handle of its current stream (the last argument of every launching entry point)."""
    import torch
    with torch.cuda.device(device):
        yield torch.cuda.current_stream(device).cuda_stream


def profile_enable(on: bool, only=None):
    """Bracket kernel launches with HIP events.  `only`: iterable of KERNEL_NAMES to restrict to (an event pair costs a few
    microseconds of stream time, so a timed region should bracket as little as it needs)."""
    mask = 0xFFFFFFFF if only is None else sum(1 << KERNEL_NAMES.index(n) for n in only)
    call(load().texgs_profile_select, mask)
    call(load().texgs_profile_enable, 1 if on else 0)


def profile_read():
    """-> {kernel_name: (total_ms, launches)} since the last read (synchronises the recorded events)."""
    n = len(KERNEL_NAMES)
    ms = (C.c_float * n)()
    cnt = (C.c_uint32 * n)()
    call(load().texgs_profile_read, ms, cnt)
    return {KERNEL_NAMES[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}
