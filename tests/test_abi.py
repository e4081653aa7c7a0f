"""-m "not gpu": the C-ABI library builds (hipcc cross-compiles without a GPU), loads, exports every symbol that
include/texgs.h declares, the ctypes mirrors in texgs/_lib.py have the C structs' sizes and field offsets, and its signature
table agrees with the header's prototypes.  No compute calls here."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "texgs.h")


def declared_functions():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(texgs_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_the_entry_points_the_host_uses():
    names = declared_functions()
    for n in ["texgs_preprocess_forward", "texgs_num_rendered_begin", "texgs_num_rendered_reduce", "texgs_depth_sort_scan",
              "texgs_bin_sort_render_forward", "texgs_render_forward", "texgs_backward", "texgs_backward_render",
              "texgs_backward_preprocess", "texgs_mark_visible", "texgs_abi_version", "texgs_last_error"]:
        assert n in names


def test_library_exports_every_declared_symbol(lib_built):
    lib = ctypes.CDLL(lib_built)
    for n in declared_functions():
        assert hasattr(lib, n), f"{n} declared in include/texgs.h but not exported by libtexgs.so"
    from texgs import _lib
    assert sorted(_lib.EXPORTS) == declared_functions()
    assert _lib.load().texgs_abi_version() == _lib.ABI_VERSION


def mirrors():
    """{C struct name: ctypes mirror} for EVERY ctypes.Structure that texgs/_lib.py defines: `Frame` mirrors `TexGSFrame`,
    `UVNetStruct` mirrors `TexGSUVNet`.  A mirror added later is picked up here without being listed."""
    from texgs import _lib
    out = {}
    for name, cls in vars(_lib).items():
        if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure:
            out["TexGS" + (name[:-len("Struct")] if name.endswith("Struct") else name)] = cls
    return out


def test_ctypes_structs_match_c_layout(tmp_path):
    from texgs import _lib
    structs = mirrors()
    assert len(structs) == 12 and {"TexGSFrame", "TexGSHashGrid", "TexGSDensityPlan", "TexGSDensityRow", "TexGSDensityMove"} <= set(structs)
    consts = {"TEXGS_ABI_VERSION": _lib.ABI_VERSION, "TEXGS_TILE": _lib.TILE, "TEXGS_REC_TEST_FLOATS": _lib.REC_TEST_FLOATS,
              "TEXGS_REC_SHADE_FLOATS": _lib.REC_SHADE_FLOATS, "TEXGS_ACC_FLOATS": _lib.ACC_FLOATS,
              "TEXGS_TEXBIN_RECORD_FLOATS": _lib.TEXBIN_RECORD_FLOATS, "TEXGS_RESV_WORDS": _lib.RESV_WORDS,
              "TEXGS_DENSITY_MAX_ROWS": _lib.DENSITY_MAX_ROWS, "TEXGS_METRICS_ROW": _lib.METRICS_ROW,
              "TEXGS_HASHGRID_MAX_LEVELS": _lib.HASHGRID_MAX_LEVELS, "TEXGS_HASHGRID_FEATURES": _lib.HASHGRID_FEATURES}
    assert abi_check.layout_mismatches("texgs.h", structs, consts, tmp_path) == []


def broken_tables_are_caught(header, signatures, mirrors, dropped, widened, swapped):
    """The check sees what it is for.  `dropped`: an entry point that loses its last argument; `widened`: (entry point, argument) of an
    int32_t stated as size_t; `swapped`: (entry point, argument, another struct's mirror) of a struct pointer."""
    def mismatches(name, k=None, t=None):
        restype, argtypes = signatures[name]
        argtypes = argtypes[:-1] if k is None else argtypes[:k] + [t] + argtypes[k + 1:]
        return abi_check.signature_mismatches(header, dict(signatures, **{name: (restype, argtypes)}), mirrors)
    protos = abi_check.prototypes(header)
    assert any(f"{dropped}: {len(protos[dropped][1])} arguments" in m for m in mismatches(dropped))
    name, k = widened
    assert protos[name][1][k] == "int32_t" and any(f"{name}: argument {k} is int32_t" in m for m in mismatches(name, k, ctypes.c_size_t))
    name, k, other = swapped
    assert any(f"{name}: argument {k} is {protos[name][1][k]}" in m for m in mismatches(name, k, ctypes.POINTER(other)))


def test_signature_table_matches_the_header():
    """texgs/_lib.py states each entry point's ctypes signature once (SIGNATURES); every one is compared with its prototype in
    include/texgs.h: the return type, the argument count, and per argument a scalar of the same width and kind, the mirror of the
    TexGS* struct pointed to, or a pointer for any other pointer (tests/abi_check.py, as every stage's test does for its own header).
    ctypes converts silently, so a wrong width or a missing argument would otherwise corrupt a call instead of failing it."""
    from texgs import _lib
    assert len(abi_check.prototypes(HDR)) == 49
    assert abi_check.signature_mismatches(HDR, _lib.SIGNATURES, mirrors()) == []
    # one argument dropped, one int32_t widened to size_t, one struct mirror swapped
    broken_tables_are_caught(HDR, _lib.SIGNATURES, mirrors(), "texgs_cube_latlong", ("texgs_scan_temp_bytes", 0),
                             ("texgs_density_move", 0, _lib.DensityPlanStruct))


def test_a_stage_headers_broken_table_is_caught_too():
    """The same three breakages against a stage's header and the table in the stage's module (texgs_params.h, texgs.params)"""
    from texgs import params
    header = os.path.join(ROOT, "include", "texgs_params.h")
    assert abi_check.signature_mismatches(header, params.SIGNATURES, params.MIRRORS) == []
    broken_tables_are_caught(header, params.SIGNATURES, params.MIRRORS, "texgs_params_activate", ("texgs_params_temp_bytes", 0),
                             ("texgs_params_covariance", 0, params.ParamsCovarianceGradStruct))
    renamed = {("texgs_params_size" if n == "texgs_params_temp_bytes" else n): v for n, v in params.SIGNATURES.items()}
    assert any("names differ" in m and "texgs_params_size" in m for m in abi_check.signature_mismatches(header, renamed, params.MIRRORS))
    void = dict(params.SIGNATURES, texgs_params_covariance=(ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]))
    assert any("texgs_params_covariance: argument 0" in m for m in abi_check.signature_mismatches(header, void, params.MIRRORS))


def test_bind_applies_a_table_once_and_names_every_missing_export(lib_built):
    """_lib.bind(table): the loaded library with the table applied; a table that names symbols the library lacks raises the rebuild
    advice with every one of them, and is not remembered; the same table a second time is the same library with argtypes as stated."""
    from texgs import _lib
    lib = _lib.load()
    absent = {"texgs_no_such_entry": (ctypes.c_int, []), "texgs_tex_bin_count": _lib.SIGNATURES["texgs_tex_bin_count"],
              "texgs_nor_this_one": (ctypes.c_int, [ctypes.c_void_p])}
    for _ in range(2):
        with pytest.raises(RuntimeError, match=r"does not export texgs_no_such_entry, texgs_nor_this_one; rebuild it with "
                                               r"`python texture-gs_amd/build.py`"):
            _lib.bind(absent)
    table = {"texgs_scan_temp_bytes": (ctypes.c_size_t, [ctypes.c_int32]), "texgs_abi_version": (ctypes.c_int, [])}
    assert _lib.bind(table) is lib and _lib.bind(table) is lib and _lib.bind(_lib.SIGNATURES) is lib
    assert lib.texgs_scan_temp_bytes.argtypes == [ctypes.c_int32] and lib.texgs_scan_temp_bytes.restype is ctypes.c_size_t
    assert lib.texgs_abi_version() == _lib.ABI_VERSION


def test_call_raises_with_the_entry_points_name(lib_built):
    """_lib.call(fn, *args): a non-zero return code becomes a RuntimeError that names the function (from the ctypes function object)
    and carries texgs_last_error(); a zero code returns quietly.  Host-only entry point: no GPU."""
    import numpy as np
    from texgs import _lib
    lib = _lib.load()
    with pytest.raises(RuntimeError, match=r"texgs_num_rendered_reduce failed \(code -1\): NULL argument"):
        _lib.call(lib.texgs_num_rendered_reduce, None, 4, None, None)
    buf = np.arange(3, dtype=np.uint32)
    d, fp = ctypes.c_uint32(0), ctypes.c_uint64(0)
    assert _lib.call(lib.texgs_num_rendered_reduce, buf.ctypes.data, 4, ctypes.byref(d), ctypes.byref(fp)) is None
    assert d.value == 0 and fp.value == (2 << 32) | 1
    import torch
    t = torch.zeros(2)
    assert _lib.ptr(None) is None and _lib.ptr(t) == t.data_ptr()


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "c.o")])


def test_num_rendered_reduce_is_host_only_arithmetic(lib_built):
    """texgs_num_rendered_words / texgs_num_rendered_reduce (the second half of the two-step instance-count readback, texgs.h) run on
    the host: D = sum of K1's per-workgroup partial sums, the fingerprint = the two wrapped 32-bit sums, an instance count past
    2^32 - 1 is an error, NULL arguments are errors.  (The first half needs a GPU: tests/test_contract_gpu.py.)"""
    import ctypes as C
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "texture-gs_amd"))
    from texgs import _lib
    lib = _lib.load()
    for N in (1, 255, 256, 257, 300_000):
        nblk = (N + 255) // 256
        assert lib.texgs_num_rendered_words(N) == 3 * nblk
        rng = np.random.RandomState(N)
        buf = np.concatenate([rng.randint(0, 5000, nblk), rng.randint(0, 2**32, nblk, dtype=np.int64),
                              rng.randint(0, 2**32, nblk, dtype=np.int64)]).astype(np.uint32)
        d, fp = C.c_uint32(0), C.c_uint64(0)
        rc = lib.texgs_num_rendered_reduce(buf.ctypes.data, N, C.byref(d), C.byref(fp))
        assert rc == 0
        assert d.value == int(buf[:nblk].astype(np.uint64).sum())
        fa = int(buf[nblk:2 * nblk].astype(np.uint64).sum()) & 0xFFFFFFFF
        fb = int(buf[2 * nblk:].astype(np.uint64).sum()) & 0xFFFFFFFF
        assert fp.value == (fb << 32) | fa
    assert lib.texgs_num_rendered_words(0) == 0 and lib.texgs_num_rendered_words(-3) == 0
    d = C.c_uint32(7)
    assert lib.texgs_num_rendered_reduce(buf.ctypes.data, 0, C.byref(d), None) == 0 and d.value == 0       # no Gaussians: D = 0
    big = np.full(3 * 2, 0xFFFFFFFF, dtype=np.uint32)                                                        # two workgroups of 2^32 - 1 each
    assert lib.texgs_num_rendered_reduce(big.ctypes.data, 512, C.byref(d), None) != 0
    assert b"2^32" in lib.texgs_last_error()
    assert lib.texgs_num_rendered_reduce(None, 4, C.byref(d), None) != 0


def test_uv_precision_is_checked_before_any_launch(lib_built):
    """The UV map's entry points take the precision as an argument (v19): texgs_uv_packed_bytes sizes the packed weights per precision,
    and a value outside TEXGS_UV_FP32 / _BF16X3 / _MIXED is refused by name before anything is launched (no GPU is needed to see it;
    a launch here would fail with a HIP error that does not name the argument)."""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, "texture-gs_amd"))
    from texgs import _lib
    lib = _lib.load()
    assert [lib.texgs_uv_packed_bytes(p) for p in (0, 1, 2)] == [196608, 196608, 393216]
    assert (_lib.UV_PRECISION["fp32"], _lib.UV_PRECISION["bf16x3"], _lib.UV_PRECISION["mixed"]) == (0, 1, 2)
    assert lib.texgs_uv_packed_bytes(3) == 0 and lib.texgs_uv_packed_bytes(-1) == 0
    net = _lib.UVNetStruct(*([None] * 13), 128)
    grads = _lib.UVNetGradStruct(*([None] * 10))
    buf = (C.c_float * 64)()          # stands in for every device buffer: nothing may read it
    b = C.addressof(buf)
    for bad in (3, -1):
        calls = {"texgs_uv_pack": lambda: lib.texgs_uv_pack(C.byref(net), bad, b, None),
                 "texgs_uv_taylor_packed": lambda: lib.texgs_uv_taylor_packed(C.byref(net), bad, b, b, 4, b, b, None),
                 "texgs_uv_backward": lambda: lib.texgs_uv_backward(C.byref(net), bad, b, b, 4, C.byref(grads), b, None)}
        for name, call in calls.items():
            assert lib.texgs_num_rendered_reduce(None, 4, None, None) != 0 and b"precision" not in lib.texgs_last_error()     # another message first
            assert call() != 0, (name, bad)
            assert b"precision" in lib.texgs_last_error(), (name, bad, lib.texgs_last_error())
    # N = 0 is a no-op whose point / output pointers may be NULL (an empty tensor's data pointer is); N < 0 is refused
    net = _lib.UVNetStruct(*([b] * 13), 128)
    for prec in (0, 1, 2):
        assert lib.texgs_uv_taylor_packed(C.byref(net), prec, b, None, 0, None, None, None) == 0, prec
        assert lib.texgs_uv_taylor_packed(C.byref(net), prec, b, None, -1, None, None, None) != 0, prec
        assert lib.texgs_uv_taylor_packed(C.byref(net), prec, b, None, 4, b, b, None) != 0 and b"NULL" in lib.texgs_last_error(), prec


def test_texture_resolution_limit_is_checked_before_any_launch(lib_built):
    """tex_res up to 7168 is accepted and 7169 refused by validate_frame, which runs before anything is launched (no GPU is needed to
    see it): the blend kernels address texels with 32-bit BYTE offsets, and 6 * 7168^2 * 12 B = 3.7e9 is below 2^32.  The
    texture-gradient bin count, which sizes tex_bin_count / tex_bin_cursor / tex_bin_base, is 301 056 there.  (The Python layer has
    no check of its own: texgs.rasterizer takes R from the texture's shape and passes it on.)"""
    import ctypes as C
    from texgs import _lib
    lib = _lib.load()
    assert 2 ** 31 < 6 * 7168 ** 2 * 12 < 2 ** 32           # (7168 = 7 * 1024, a round number below sqrt(2^32 / 72) = 7723)
    assert 6 * 7168 ** 2 * 12 - 12 == 3699376116
    assert [int(lib.texgs_tex_bin_count(R)) for R in (1, 32, 33, 2336, 2368, 5462, 7168)] == [6, 6, 24, 31974, 32856, 175446, 301056]
    buf = (C.c_float * 64)()              # stands in for every device pointer of the frame: a refused call reads none of them
    b = C.addressof(buf)
    frame = lambda R, N=0: _lib.Frame(16, 16, 1.0, 1.0, 1.0, 0, 0, R, N, 0, b, b, b, b)
    inputs = _lib.Inputs(*([None] * 10))
    geom = _lib.Geom(*([None] * 8), 0)
    binning = _lib.Binning(0, None, None, None, None, None, None, 0)
    image = _lib.Image(*([None] * 11))
    assert lib.texgs_preprocess_forward(C.byref(frame(7168)), C.byref(inputs), C.byref(geom), None) == 0      # no Gaussians: valid, nothing to launch
    for call in (lambda: lib.texgs_preprocess_forward(C.byref(frame(7169)), C.byref(inputs), C.byref(geom), None),
                 lambda: lib.texgs_preprocess_forward(C.byref(frame(7169, 5)), C.byref(inputs), C.byref(geom), None),
                 lambda: lib.texgs_render_forward(C.byref(frame(7169, 5)), C.byref(inputs), C.byref(geom), C.byref(binning), C.byref(image), None)):
        assert lib.texgs_num_rendered_reduce(None, 4, None, None) != 0 and b"7168" not in lib.texgs_last_error()     # another message first
        assert call() != 0
        assert b"tex_res > 7168" in lib.texgs_last_error() and b"32-bit byte offsets" in lib.texgs_last_error()
    with pytest.raises(RuntimeError, match=r"texgs_render_forward failed .*tex_res > 7168"):
        _lib.call(lib.texgs_render_forward, C.byref(frame(7169, 5)), C.byref(inputs), C.byref(geom), C.byref(binning), C.byref(image), None)


def test_every_unit_refuses_into_the_one_error_string(lib_built):
    """Each unit that defines entry points refuses one call before any launch (no GPU is needed: nothing reads the stand-in buffer),
    with a non-zero code and its own text in texgs_last_error().  The error string is abi.hip's alone: the calls go through the units
    forwards and then backwards, every text differs from the one before it, so a unit that wrote to a copy of its own would be seen."""
    import ctypes as C
    raw = C.CDLL(lib_built)
    raw.texgs_last_error.restype = C.c_char_p
    buf = (C.c_float * 64)()
    b = C.c_void_p(C.addressof(buf))
    f, d, i64 = C.c_float, C.c_double, C.c_int64
    refusals = [
        ("abi.hip", lambda: raw.texgs_preprocess_forward(None, None, None, None), b"frame is NULL"),
        ("loss.hip", lambda: raw.texgs_geom_losses(None, None, None, None, None, None, 0, 8, f(0), f(0), f(1), f(0), b, None, None, None),
         b"image size and gamma must be positive"),
        ("uvnet.hip", lambda: raw.texgs_uv_pack(b, 99, b, None), b"precision must be TEXGS_UV_FP32, TEXGS_UV_BF16X3 or TEXGS_UV_MIXED"),
        ("uvmap.hip", lambda: raw.texgs_hashgrid_forward(None, b, b, 4, b, None), b"grid is NULL"),
        ("points.hip", lambda: raw.texgs_farthest_points(b, 0, 1, 0, b, b, None), b"n < 1"),
        ("cubetex.hip", lambda: raw.texgs_cube_sample(b, 1, 3, b, 4, 0, 0, b, None), b"R < 2: a cubemap face needs at least 2 x 2 texels"),
        ("density.hip", lambda: raw.texgs_density_stats(b, b, -1, b, b, b, None), b"n < 0"),
        ("metrics.hip", lambda: raw.texgs_eval_metrics(b, b, None, None, None, 3, 8, 0, b, b, None),
         b"H and W must be at least 7: the 7x7 SSIM window does not fit"),
        ("selftest.hip", lambda: raw.texgs_selftest_waveops(None, None, None), b"NULL argument"),
        ("optim.hip", lambda: raw.texgs_adam_step(None, -1, 0, None), b"count < 0"),
        ("mlp.hip", lambda: raw.texgs_mlp_forward(None, b, b, 4, b, b, None), b"mlp is NULL"),
        ("present.hip", lambda: raw.texgs_present(None, None), b"present descriptor is NULL"),
        ("ingest.hip", lambda: raw.texgs_rgba_composite(b, b, 20000, 4, d(0), d(0), d(0), None),
         b"20000 x 4: an image side above 16384 is not supported"),
        ("surface.hip", lambda: raw.texgs_surface_compose(None, None), b"compose descriptor is NULL"),
        ("lpips.hip", lambda: raw.texgs_conv3x3_pack(b, 0, 16, 0, b, None), b"Cin must be in [1,512], got 0"),
        ("lpips_grad.hip", lambda: raw.texgs_lpips_gate(b, b, i64(0), None), b"n must be in [1,2^40), got 0"),
        ("params.hip", lambda: raw.texgs_params_activate(None, None, C.c_size_t(0), None), b"activate descriptor is NULL"),
        ("retexture.hip", lambda: raw.texgs_retexture_cross(None, None), b"retexture cross descriptor is NULL"),
        ("shcolor.hip", lambda: raw.texgs_sh_colors_forward(None, None, 1, None), b"sh colours descriptor is NULL"),
    ]
    build = abi_check.build_script()
    assert sorted(u for u, _, _ in refusals) == sorted(set(build.UNITS) - {"preprocess.hip", "binning.hip", "render.hip"})
    assert len({text for _, _, text in refusals}) == len(refusals)
    for unit, call, text in refusals + refusals[-2::-1]:
        assert raw.texgs_last_error() != text, unit
        assert call() != 0, unit
        assert raw.texgs_last_error() == text, (unit, raw.texgs_last_error())


def unit_of(header, name):
    """The unit that defines an entry point: a stage's header names its unit; texgs.h is shared by the stages older than that rule"""
    if header == "texgs_multiview.h":
        return "abi.hip"
    if header != "texgs.h":
        return header[len("texgs_"):-len(".h")] + ".hip"
    for unit, names in {"loss.hip": r"rgb_alpha_loss|geom_losses|norm_from_depth", "uvnet.hip": r"uv_\w+", "uvmap.hip": r"hashgrid_\w+|chamfer_nn\w*",
                        "points.hip": r"knn3_\w+|fps_temp_bytes|farthest_points", "cubetex.hip": r"cube_\w+", "density.hip": r"density_\w+",
                        "metrics.hip": r"eval_metrics\w*", "selftest.hip": r"selftest_waveops"}.items():
        if re.fullmatch("texgs_(?:%s)" % names, name):
            return unit
    return "abi.hip"


def test_each_prototype_is_defined_in_its_own_unit():
    """Every function that a header of include/ declares is defined in exactly one file of csrc/: the unit of its stage, where its
    launcher and its argument checks are; abi.hip has the rasterizer's (K1-K8, the batched front end, the SH flush)."""
    csrc = os.path.join(ROOT, "texture-gs_amd", "csrc")
    code = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    headers = sorted(h for h in os.listdir(abi_check.INC) if h.endswith(".h"))
    assert len(headers) == 12
    seen = 0
    for header in headers:
        for name in abi_check.prototypes(os.path.join(abi_check.INC, header)):
            definition = re.compile(r'^(?:extern "C" )?(?:const )?\w+\s*\*?\s*%s\s*\([^;{}]*\)\s*\{' % name, re.M)       # at the start of a line, with a body
            assert [f for f, text in code.items() if definition.search(text)] == [unit_of(header, name)], (header, name)
            seen += 1
    assert seen == 88
    assert unit_of("texgs.h", "texgs_mark_visible") == "abi.hip" and unit_of("texgs_present.h", "texgs_cube_cross") == "present.hip"
