"""-m "not gpu": the retexture stage (texgs/retexture.py, include/texgs_retexture.h, csrc/retexture_math.h) without a GPU.

* The statement (tests/retexture_ref.py) against its host anchors: `cross_new_u8` equals `texture_io.resize_bilinear_u8` of the
  whole cross byte for byte; `mode_tail` equals the reference's own `change_texture` results (tests/golden/texture_io.npz) bit for
  bit and `texture_io.change_texture` (torch) on inputs either side of every branch.
* The kernels' per-texel arithmetic (csrc/retexture_math.h) compiled for the host with g++ equals the statement bit for bit.
* Structure: the header as C99 and pedantic C++, the ctypes mirrors against gcc's layout, the exports, every refusal of the C entries
  (they need no GPU) and of the Python layer, each by name.
* The lat-long statement: a constant picture, the wrap at the seam, the orientation against cubetex's own direction table."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import retexture_ref as R  # noqa: E402
from texgs import retexture as RT  # noqa: E402  (the feature under test: without it this file fails at import)
from texgs import texture_io as TIO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_retexture.h")
CSRC = os.path.join(ROOT, "texture-gs_amd", "csrc")
G = np.load(os.path.join(ROOT, "tests", "golden", "texture_io.npz"))
F = np.float32
PAIRS = [(12, 12), (7, 5), (3, 8), (1, 4), (5, 33), (40, 17)]          # (r, R)


def _faces(cross):
    return TIO.cross_to_cube(torch.from_numpy(cross)).numpy()


# ---- the statement against its host anchors ----
@pytest.mark.parametrize("r,R_", PAIRS)
def test_cross_new_u8_equals_the_host_resize_cut_into_faces(r, R_):
    cross = R.hard_cross(r, seed=100 + r)
    pos = np.array(R.CROSS_POS)
    cells = np.zeros((3, 4), bool)
    cells[pos[:, 0], pos[:, 1]] = True
    unused = np.repeat(np.repeat(~cells, r, 0), r, 1)
    assert cross[unused].any()                      # non-zero unused cells: a tap across a cell border reads them
    want = _faces(TIO.resize_bilinear_u8(cross, 3 * R_, 4 * R_))
    got = R.cross_new_u8(cross, R_, "rgb")
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # bgr: the source holds b, g, r; the texture gets r, g, b
    assert np.array_equal(R.cross_new_u8(np.ascontiguousarray(cross[..., ::-1]), R_, "bgr"), want)
    # a texel list gives the same values as the whole array
    t = R.all_texels(R_)[:: max(1, R_ // 2)]
    assert np.array_equal(R.cross_new_u8(cross, R_, "rgb", t), want[t[:, 0], t[:, 1], t[:, 2]])


@pytest.mark.parametrize("mode", R.MODES)
def test_mode_tail_equals_the_reference_results_bit_for_bit(mode):
    new01 = _faces(G["cross_u8"]).astype(F) / F(255.0)
    got = R.mode_tail(G["texture0"], new01, mode)
    assert R.same_class_and_bits(got, G[f"change_texture_m{mode + 1}"])
    # the same through the whole cross path at r = R: the host's img.copy() branch
    assert R.same_class_and_bits(R.retexture_cross(G["texture0"], G["cross_u8"], mode), G[f"change_texture_m{mode + 1}"])


def _same_finite_close_and_same_specials(got, want, rtol=1e-6):
    got, want = np.asarray(got, F), np.asarray(want, F)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(np.sign(got[inf]), np.sign(want[inf]))
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=1e-6)


@pytest.mark.parametrize("mode", R.MODES)
def test_mode_tail_against_change_texture_in_torch(mode):
    """Black texels (x/0 and 0/0 in mode 2) and 8-bit channel sums of 2 and 3, the two sides of mode 3's 0.01"""
    Rr = 9
    cross = R.hard_cross(Rr, seed=7)
    tex = R.hard_texture(Rr, seed=8)
    faces = _faces(cross)
    sums = faces.astype(np.int64).sum(-1)
    assert (sums == 0).any() and (sums == 2).any() and (sums == 3).any()
    new01 = faces.astype(F) / F(255.0)
    want = TIO.change_texture(torch.from_numpy(tex), torch.from_numpy(cross.astype(F) / F(255.0)), mode).numpy()
    got = R.mode_tail(tex, new01, mode)
    if mode == 2:
        assert np.isinf(want).any() and np.isnan(want).any()
    _same_finite_close_and_same_specials(got, want)


# ---- the kernels' arithmetic, compiled for the host ----
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "retexture_math.h"
namespace rm = retexture_math;
// in: int32 r, R, order; uint8 cross[3r*4r*3]; float old[6*R*R*3]
// out: uint8 new[6*R*R*3]; then for the modes -1..3 float tex[6*R*R*3]
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    int32_t hd[3];
    if (!f || fread(hd, 4, 3, f) != 3) return 1;
    const int32_t r = hd[0], R = hd[1], order = hd[2];
    std::vector<uint8_t> cross((size_t)36 * r * r);
    std::vector<float> old((size_t)18 * R * R);
    if (fread(cross.data(), 1, cross.size(), f) != cross.size() || fread(old.data(), 4, old.size(), f) != old.size()) return 1;
    fclose(f);
    const double sx = (double)(4 * r) / (double)(4 * R), sy = (double)(3 * r) / (double)(3 * R);
    std::vector<uint8_t> nw(old.size());
    std::vector<float> tex(5 * old.size());
    size_t t = 0;
    for (int fc = 0; fc < 6; ++fc)
        for (int y = 0; y < R; ++y)
            for (int x = 0; x < R; ++x, ++t) {
                const rm::Tap ty = rm::cross_tap(rm::cross_row(fc) * R + y, 3 * r, sy);
                const rm::Tap tx = rm::cross_tap(rm::cross_col(fc) * R + x, 4 * r, sx);
                const uint8_t* r0 = cross.data() + (size_t)3 * ty.i0 * 4 * r;
                const uint8_t* r1 = cross.data() + (size_t)3 * ty.i1 * 4 * r;
                float n[3];
                for (int ch = 0; ch < 3; ++ch) {
                    const int sc = order ? 2 - ch : ch;
                    nw[3 * t + ch] = rm::cross_blend(r0[3 * tx.i0 + sc], r0[3 * tx.i1 + sc], r1[3 * tx.i0 + sc], r1[3 * tx.i1 + sc], tx.w, ty.w);
                    n[ch] = rm::unit_of_byte(nw[3 * t + ch]);
                }
                for (int mode = -1; mode <= 3; ++mode) rm::mode_tail(&old[3 * t], n, mode, &tex[(size_t)(mode + 1) * old.size() + 3 * t]);
            }
    f = fopen(argv[2], "wb");
    fwrite(nw.data(), 1, nw.size(), f);
    fwrite(tex.data(), 4, tex.size(), f);
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("retexture_math")
    src, exe = d / "harness.cpp", d / "harness"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    return exe


@pytest.mark.parametrize("r,R_", PAIRS)
def test_arithmetic_of_the_kernels_equals_the_statement_bit_for_bit(harness, tmp_path, r, R_):
    """csrc/retexture_math.h is what the kernels compute per texel; built here for the host without contraction, as build.py builds it
    for the device: the taps, the fp64 blend, the quantisation and the five tails."""
    for order in ("rgb", "bgr"):
        cross, tex = R.hard_cross(r, seed=100 + r), R.hard_texture(R_, seed=200 + R_)
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([r, R_, order == "bgr"], np.int32).tobytes() + cross.tobytes() + tex.tobytes())
        subprocess.check_call([str(harness), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        raw = open(tmp_path / "out.bin", "rb").read()
        n = tex.size
        assert len(raw) == n + 5 * 4 * n
        new = np.frombuffer(raw[:n], np.uint8).reshape(tex.shape)
        want_new = R.cross_new_u8(cross, R_, order)
        assert np.array_equal(new, want_new)
        got = np.frombuffer(raw[n:], F).reshape((5,) + tex.shape)
        for mode in R.MODES:
            assert R.same_class_and_bits(got[mode + 1], R.mode_tail(tex, R.new01_of_u8(want_new), mode)), (order, mode)
    if (r, R_) == (12, 12):         # the golden case through the compiled arithmetic
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([12, 12, 0], np.int32).tobytes() + G["cross_u8"].tobytes() + G["texture0"].tobytes())
        subprocess.check_call([str(harness), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        got = np.frombuffer(open(tmp_path / "out.bin", "rb").read()[G["texture0"].size:], F).reshape((5,) + G["texture0"].shape)
        for mode in R.MODES:
            assert R.same_class_and_bits(got[mode + 1], G[f"change_texture_m{mode + 1}"]), mode


# ---- structure ----
def test_header_compiles_as_c_and_as_cpp_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_retexture.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "texgs_retexture.h"\nint main(){return 0;}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "cpp.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert "TEXGS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "texgs_retexture.h"' in open(os.path.join(CSRC, "retexture.hip")).read()
    assert re.search(r"#define TEXGS_ABI_VERSION 19\b", open(os.path.join(INC, "texgs.h")).read())
    for name in ("retexture.hip", "retexture_math.h"):         # the kernels: plain C++, no inline assembly, no atomics, no LDS
        code = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"\basm\b|__asm|atomic[A-Z_a-z]*\(|__shared__", code), name
    build = abi_check.build_knows_header(HDR)
    assert build.UNITS["retexture.hip"] == ["-ffp-contract=off"]


def test_structs_match_c_layout(tmp_path):
    consts = {"TEXGS_RETEX_TEXELS_PER_THREAD": RT.TEXELS_PER_THREAD, "TEXGS_RETEX_THREADS": RT.THREADS, "TEXGS_RETEX_MAX_RES": RT.MAX_RES,
              "TEXGS_RETEX_MAX_SRC": RT.MAX_SRC, "TEXGS_RETEX_RGB": RT.ORDERS["rgb"], "TEXGS_RETEX_BGR": RT.ORDERS["bgr"]}
    assert sorted(RT.MIRRORS) == ["TexGSRetexCross", "TexGSRetexLatLong"]
    assert abi_check.layout_mismatches("texgs_retexture.h", RT.MIRRORS, consts, tmp_path) == []


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(RT.SIGNATURES) == ["texgs_retexture_cross", "texgs_retexture_latlong"]
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, RT.SIGNATURES, RT.MIRRORS) == []
    lib = RT.entry()
    assert lib is _lib.load() and lib.texgs_retexture_cross.argtypes == RT.SIGNATURES["texgs_retexture_cross"][1]
    assert lib.texgs_abi_version() == 19
    assert not any(n in _lib.SIGNATURES for n in protos)        # the table of _lib.py is texgs.h alone (tests/test_abi.py)


def test_c_entries_refuse_bad_arguments_before_any_launch(lib_built):
    """No GPU here: a call that got as far as a launch would fail with a HIP error instead of the cause named below."""
    lib = RT.entry()
    buf = (C.c_double * 4096)()             # stands in for every device buffer: nothing may read it
    b = (C.addressof(buf) + 15) & ~15
    tex_bytes = 6 * 2 * 2 * 12              # R = 2
    src, old, out = b, b + 1024, b + 2048
    err = lambda: lib.texgs_last_error().decode()
    X = lambda **kw: RT.RetexCrossStruct(**{**dict(src=src, old_tex=old, out_tex=out, r=1, R=2, mode=0, order=0), **kw})
    L = lambda **kw: RT.RetexLatLongStruct(**{**dict(src=src, old_tex=old, out_tex=out, h=2, w=4, R=2, mode=0, src_u8=0), **kw})
    common = [
        (dict(src=None), "NULL argument (src)"), (dict(out_tex=None), "NULL argument (out_tex)"),
        (dict(old_tex=None), "NULL argument (old_tex)"), (dict(old_tex=None, mode=3), "NULL argument (old_tex)"),
        (dict(R=0), "R must be in [1,7168]"), (dict(R=7169), "R must be in [1,7168]"), (dict(R=-4), "R must be in [1,7168]"),
        (dict(mode=4), "mode must be -1, 0, 1, 2 or 3"), (dict(mode=-2), "mode must be -1, 0, 1, 2 or 3"),
        (dict(old_tex=old + 2), "4-byte aligned"), (dict(out_tex=out + 1), "4-byte aligned"),
        (dict(out_tex=old + 12), "out_tex overlaps old_tex"), (dict(out_tex=old - 12), "out_tex overlaps old_tex"),
        (dict(out_tex=old + tex_bytes - 4), "out_tex overlaps old_tex"), (dict(out_tex=src), "out_tex overlaps src"),
    ]
    for mk, fn, own in [
            (X, lib.texgs_retexture_cross, [(dict(r=0), "r must be in [1,16384]"), (dict(r=16385), "r must be in [1,16384]"),
                                            (dict(order=2), "order must be 0 (rgb) or 1 (bgr)"), (dict(order=-1), "order must be"),
                                            (dict(out_tex=src + 32, old_tex=None, mode=-1), "out_tex overlaps src")]),
            (L, lib.texgs_retexture_latlong, [(dict(h=0), "h and w must be in [1,16384]"), (dict(w=16385), "h and w must be in [1,16384]"),
                                              (dict(src_u8=2), "src_u8 must be 0 or 1"), (dict(src=src + 2), "a float src must be 4-byte aligned"),
                                              (dict(out_tex=src + 92, old_tex=None, mode=-1), "out_tex overlaps src")])]:
        for kw, cause in common + own:
            assert fn(C.byref(mk(**kw)), None) != 0, kw
            assert cause in err(), (kw, err())
        assert fn(None, None) != 0 and "descriptor is NULL" in err()
    # mode -1 does without the old texture, and a byte picture needs no alignment: these are refused for the NEXT cause only
    assert lib.texgs_retexture_cross(C.byref(X(old_tex=None, mode=-1, out_tex=None)), None) != 0 and "NULL argument (out_tex)" in err()
    assert lib.texgs_retexture_latlong(C.byref(L(src=src + 1, src_u8=1, old_tex=None, mode=-1, out_tex=None)), None) != 0 \
        and "NULL argument (out_tex)" in err()
    # out_tex just past old_tex is no overlap (refused for the next cause, again)
    assert lib.texgs_retexture_cross(C.byref(X(out_tex=old + tex_bytes, mode=7)), None) != 0 and "mode must be" in err()


def test_every_validation_error_comes_before_the_cpu_refusal(tmp_path):
    tex, cross = torch.zeros(6, 4, 4, 3), torch.zeros(6, 8, 3, dtype=torch.uint8)
    pic = torch.zeros(4, 8, 3)
    cr = lambda texture_sh0=tex, cross_u8=cross, **kw: RT.retexture_cross_u8(texture_sh0, cross_u8, **kw)
    ll = lambda latlong=pic, **kw: RT.retexture_latlong(latlong, **kw)
    png = str(tmp_path / "bad.png")
    from PIL import Image
    Image.fromarray(np.zeros((6, 9, 3), np.uint8), "RGB").save(png)
    bad = [
        (TypeError, "texture_sh0 must be a torch.Tensor", lambda: cr(texture_sh0=np.zeros((6, 4, 4, 3), F))),
        (ValueError, r"texture_sh0 must be \[6,R,R,3\]", lambda: cr(texture_sh0=torch.zeros(6, 4, 5, 3))),
        (ValueError, r"texture_sh0 must be \[6,R,R,3\]", lambda: cr(texture_sh0=torch.zeros(6, 4, 4, 4))),
        (ValueError, "texture_sh0 must be torch.float32", lambda: cr(texture_sh0=tex.double())),
        (ValueError, "texture_sh0 must be contiguous", lambda: cr(texture_sh0=torch.zeros(6, 4, 4, 6)[..., ::2])),
        (TypeError, "cross_u8 must be a torch.Tensor", lambda: cr(cross_u8=None)),
        (ValueError, "cross_u8 must be torch.uint8", lambda: cr(cross_u8=cross.float())),
        (ValueError, r"a cubemap cross must be \[3r,4r,3\]", lambda: cr(cross_u8=torch.zeros(6, 9, 3, dtype=torch.uint8))),
        (ValueError, r"a cubemap cross must be \[3r,4r,3\]", lambda: cr(cross_u8=torch.zeros(6, 8, dtype=torch.uint8))),
        (ValueError, "cross_u8 must be contiguous", lambda: cr(cross_u8=torch.zeros(6, 8, 6, dtype=torch.uint8)[..., ::2])),
        (TypeError, "mode must be an int", lambda: cr(mode=1.0)), (TypeError, "mode must be an int", lambda: cr(mode=True)),
        (ValueError, "mode must be -1, 0, 1, 2 or 3", lambda: cr(mode=4)), (ValueError, "mode must be -1, 0, 1, 2 or 3", lambda: cr(mode=-2)),
        (ValueError, "order must be 'rgb' or 'bgr'", lambda: cr(order="gbr")), (ValueError, "order must be 'rgb' or 'bgr'", lambda: cr(order=1)),
        (ValueError, r"out must be \[6,4,4,3\]", lambda: cr(out=torch.zeros(6, 5, 5, 3))),
        (ValueError, "out must be torch.float32", lambda: cr(out=tex.double())),
        (TypeError, "latlong must be a torch.Tensor", lambda: ll(latlong=np.zeros((4, 8, 3), F), R=4)),
        (ValueError, "latlong must be torch.float32 or torch.uint8", lambda: ll(latlong=pic.double(), R=4)),
        (ValueError, r"latlong must be \[h,w,3\]", lambda: ll(latlong=torch.zeros(4, 8, 4), R=4)),
        (ValueError, r"latlong must be \[h,w,3\]", lambda: ll(latlong=torch.zeros(0, 8, 3), R=4)),
        (ValueError, "latlong must be contiguous", lambda: ll(latlong=torch.zeros(4, 8, 6)[..., ::2], R=4)),
        (ValueError, "the texture resolution is unknown", lambda: ll()),
        (TypeError, "R must be an int", lambda: ll(R=4.0)), (ValueError, r"R must be in \[1,7168\]", lambda: ll(R=0)),
        (ValueError, r"R must be in \[1,7168\]", lambda: ll(R=7169)),
        (ValueError, "mismatched resolutions", lambda: ll(R=5, texture_sh0=tex, mode=0)),
        (ValueError, "mismatched resolutions", lambda: ll(texture_sh0=tex, out=torch.zeros(6, 5, 5, 3))),
        (ValueError, "texture_sh0 is needed by mode 0", lambda: ll(R=4, mode=0)),
        (ValueError, "mode must be -1, 0, 1, 2 or 3", lambda: ll(R=4, mode=9)),
        (ValueError, r"texture_sh0 must be \[6,R,R,3\]", lambda: RT.retexture_png(torch.zeros(5, 4, 4, 3), png)),
        (ValueError, "mode must be -1, 0, 1, 2 or 3", lambda: RT.retexture_png(tex, png, mode=5)),
    ]
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()
    # valid arguments on the CPU: refused as such and by the function's name, never computed in torch
    for name, call in (("retexture_cross_u8", lambda: cr()), ("retexture_cross_u8", lambda: cr(mode=3, order="bgr", out=tex)),
                       ("retexture_latlong", lambda: ll(R=4)), ("retexture_latlong", lambda: ll(latlong=pic.to(torch.uint8), texture_sh0=tex, mode=2)),
                       ("retexture_png", lambda: RT.retexture_png(tex, png))):
        with pytest.raises(RuntimeError, match=rf"texgs\.retexture\.{name}: .* no CPU fallback"):
            call()
    assert RT.retexture_cross_u8.__doc__ and "differentiable" in RT.retexture_cross_u8.__doc__ and "UNPINNED" in RT.__doc__


# ---- the lat-long statement ----
def test_latlong_of_a_constant_picture_is_that_constant():
    pic = np.full((5, 7, 3), F(0.625))
    for fn in (R.latlong_f64, R.latlong_mixed):
        out = fn(pic, 6)
        np.testing.assert_allclose(out, (0.625 - 0.5) / 0.28209479177387814, rtol=0, atol=1e-6)
    u8 = np.full((4, 8, 3), 51, np.uint8)
    np.testing.assert_allclose(R.latlong_f64(u8, 3), (0.2 - 0.5) / 0.28209479177387814, rtol=0, atol=1e-12)


def test_latlong_wraps_at_the_seam():
    R_, h, w = 64, 16, 32
    at, wx = R.seam_texels(R_, h, w)
    assert len(at) >= R_ and (at[:, 1] < R_ // 2).any() and (at[:, 1] >= R_ // 2).any()       # both sides of the seam
    got = R.latlong_f64(R.seam_picture(h, w), R_)[R.SEAM_FACE][at[:, 0], at[:, 1]] * 0.28209479177387814 + 0.5
    # a blend of the LAST column (0) and the FIRST (1) with weight wx: a clamped axis would give 0 or 1, never the blend
    np.testing.assert_allclose(got, np.repeat(wx[:, None], 3, 1), rtol=0, atol=1e-12)
    assert ((wx > 0.05) & (wx < 0.95)).any()


def test_latlong_orientation_round_trip_through_cubetex_directions():
    """Six faces of distinct constant colours through cubetex's own lat-long direction table (its float64 host form) at 256 x 512, and
    back at R = 8: the central 4 x 4 of every face returns that face's colour"""
    from texgs import cubetex
    dirs = cubetex.latlong_dirs((256, 512), "cpu").double().numpy()
    pic = R.FACE_COLOURS[R.face_of(dirs)]
    for fn in (R.latlong_f64, R.latlong_mixed):
        rgb = fn(pic, 8) * 0.28209479177387814 + 0.5
        for f in range(6):
            np.testing.assert_allclose(rgb[f, 2:6, 2:6], np.broadcast_to(R.FACE_COLOURS[f], (4, 4, 3)), rtol=0, atol=1e-6, err_msg=str(f))
