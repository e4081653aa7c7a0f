"""-m "not gpu": the colour stage (texgs/shcolor.py, include/texgs_shcolor.h, csrc/shcolor_math.h) without a GPU.

* The float64 statement (tests/shcolor_ref.py) against what the reference's own code computed in float64, values and autograd
  gradients (tests/golden/shcolor.npz, recorded by tests/golden/make_shcolor_golden.py), to 1e-12.
* The float32 statement of eval_sh against the reference's float32 CPU results on the same directions, bit for bit, degrees 0..4;
  the clamp's edge on the constructed degree-0 rows.
* The kernels' row arithmetic (csrc/shcolor_math.h) compiled for the host with g++ against the float32 statement, bit for bit.
* Structure: the ctypes mirrors against gcc's layout of the header's structs, the header as C and as C++, the exports and their
  signatures against the prototypes, the C entries' refusals (they need no GPU), the build script's knowledge of the unit.
* Every validation error of texgs.shcolor is raised on CPU tensors BEFORE the "no CPU fallback" error."""
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
import shcolor_ref as R  # noqa: E402
from texgs import shcolor as _shcolor  # noqa: E402,F401  (the feature under test: without it this file fails at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_shcolor.h")
CSRC = os.path.join(ROOT, "texture-gs_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "shcolor.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ---- the statement ----
def test_float64_statement_equals_the_reference_in_float64(golden):
    """Values and every gradient to 1e-12 of each field's scale (shcolor_ref.backward_scales; sum_k |sh[k]| + 1 for the values)"""
    G = golden
    sh, xyz, cam, g = (G[k].astype(np.float64) for k in ("features", "xyz", "campos", "g"))
    N, K = sh.shape[:2]
    tol = 1e-12
    for deg in range(5):
        A = (deg + 1) ** 2
        vscale = np.abs(sh[:, :A]).sum(axis=1) + 1.0
        assert R.max_error(R.S64.colors(deg, sh, xyz, cam), G[f"colors64_{deg}"], vscale) <= tol, deg
        d_sh, d_xyz = R.S64.colors_backward(deg, sh, xyz, cam.reshape(1, 3), g[None])
        s_sh, s_xyz = R.backward_scales(deg, sh, xyz, cam.reshape(1, 3), g[None])
        assert R.max_error(d_sh[:, :A], G[f"d_sh64_{deg}"], s_sh[:, :A]) <= tol, deg
        assert not d_sh[:, A:].any()
        assert R.max_error(d_xyz, G[f"d_xyz64_{deg}"], s_xyz) <= tol, deg
        if deg:
            assert np.abs(G[f"d_xyz64_{deg}"]).max() > 1e-3             # (the comparison above is of something)
        dirs = G[f"dirs32_{deg}"].astype(np.float64)
        assert R.max_error(R.S64.eval_sh(deg, sh, dirs), G[f"eval64_{deg}"], vscale) <= tol, deg
        e_sh, e_dirs = R.S64.eval_sh_backward(deg, sh, dirs, g)
        assert R.max_error(e_dirs, G[f"d_dirs64_{deg}"], s_xyz * np.linalg.norm(xyz - cam, axis=1, keepdims=True)) <= tol, deg
        b = R.S64.basis(deg, dirs[:, 0], dirs[:, 1], dirs[:, 2])
        assert all(np.array_equal(e_sh[:, k], b[k][:, None] * g) for k in range(A)) and not e_sh[:, A:].any()
    # two views sum: the statement's view loop against the sum of two one-view calls (float64: the order does not show at 1e-12)
    cams = np.stack([cam, cam + 0.25])
    g2 = np.stack([g, g[::-1]])
    both = R.S64.colors_backward(3, sh, xyz, cams, g2)
    one = [R.S64.colors_backward(3, sh, xyz, cams[v:v + 1], g2[v:v + 1]) for v in range(2)]
    s_sh, s_xyz = R.backward_scales(3, sh, xyz, cams, g2)
    assert R.max_error(both[0], one[0][0] + one[1][0], s_sh) <= tol and R.max_error(both[1], one[0][1] + one[1][1], s_xyz) <= tol


def test_float32_statement_of_eval_sh_equals_the_reference_bit_for_bit(golden):
    G = golden
    sh = G["features"]
    for deg in range(5):
        got = R.S32.eval_sh(deg, sh, G[f"dirs32_{deg}"])
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), G[f"eval32_{deg}"].view(np.uint32)), deg
        col = R.S32.clamp(got)
        assert np.array_equal(col.view(np.uint32), G[f"colors32_{deg}"].view(np.uint32)), deg
        clamped = float((col == 0).mean())
        print(f"degree {deg}: {100 * clamped:.1f} % clamped")
        assert 0.01 <= clamped <= 0.5
    # the direction is this project's statement, not torch's: the two norms differ by at most one unit in the last place (a sum
    # of three squares associated differently under one square root), so the quotients differ by at most two of theirs
    d, _ = R.S32.direction(G["xyz"], G["campos"])
    ulp = np.spacing(np.abs(G["dirs32_3"]))
    off = np.abs(d.astype(np.float64) - G["dirs32_3"]) / ulp
    print("direction against torch's: largest difference in ulp", off.max(), "rows that differ", float((off > 0).any(axis=1).mean()))
    assert off.max() <= 2.0


def test_clamp_passes_the_gradient_at_exactly_zero(golden):
    """The constructed degree-0 rows: around the float32 coefficient whose C0 * s + 0.5 is exactly zero, torch's clamp_min gives a
    zero colour with a NON-zero gradient at the exact row, zero gradient below it"""
    G = golden
    s, exact = G["edge_sh"], G["edge_exact"]
    assert exact.sum() >= 1 and (G["edge_color"][exact] == 0).all() and (G["edge_grad"][exact] != 0).all()
    M = s.size
    sh = np.repeat(s.reshape(M, 1, 1), 3, axis=2)
    xyz, cam = np.ones((M, 3), R.F), np.zeros(3, R.F)
    col = R.S32.colors(0, sh, xyz, cam)
    assert np.array_equal(col[:, 0].view(np.uint32), G["edge_color"].view(np.uint32))
    g = np.zeros((1, M, 3), R.F)
    g[0, :, 0] = 1
    d_sh, d_xyz = R.S32.colors_backward(0, sh, xyz, cam.reshape(1, 3), g)
    assert np.array_equal(d_sh[:, 0, 0].view(np.uint32), G["edge_grad"].view(np.uint32))
    assert (d_sh[:, 0, 0] == 0).any() and (d_sh[:, 0, 0] != 0).any() and not d_xyz.any() and not d_sh[:, 0, 1:].any()


HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "shcolor_math.h"
namespace sm = shcolor_math;
static std::vector<float> rd(FILE* f, size_t n) { std::vector<float> v(n); if (n && fread(v.data(), 4, n, f) != n) exit(3); return v; }
static void wr(FILE* f, const std::vector<float>& v) { if (v.size() && fwrite(v.data(), 4, v.size(), f) != v.size()) exit(4); }
template <int DEG>
static void run(size_t N, size_t V, bool eval_mode, const std::vector<float>& sh, const std::vector<float>& xyz, const std::vector<float>& cams,
                const std::vector<float>& g, std::vector<float>& col, std::vector<float>& d_sh, std::vector<float>& d_xyz) {
    constexpr int W = 3 * sm::coeffs_of(DEG);
    for (size_t i = 0; i < N; ++i) {
        float acc[W], ax[3] = {0.0f, 0.0f, 0.0f};
        for (int j = 0; j < W; ++j) acc[j] = 0.0f;
        for (size_t v = 0; v < V; ++v) {
            sm::row_forward<DEG>(&sh[W * i], &xyz[3 * i], &cams[3 * v], eval_mode, &col[3 * (v * N + i)]);
            sm::row_backward_view<DEG>(&sh[W * i], &xyz[3 * i], &cams[3 * v], &g[3 * (v * N + i)], eval_mode, true, true, acc, ax);
        }
        for (int j = 0; j < W; ++j) d_sh[W * i + j] = acc[j];
        for (int j = 0; j < 3; ++j) d_xyz[3 * i + j] = ax[j];
    }
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h[4];
    if (fread(h, 4, 4, f) != 4) return 3;
    const int deg = h[0];
    const size_t N = (size_t)h[1], V = (size_t)h[2], W = 3 * (size_t)sm::coeffs_of(deg);
    const bool eval_mode = h[3] != 0;
    auto sh = rd(f, N * W), xyz = rd(f, 3 * N), cams = rd(f, 3 * V), g = rd(f, 3 * V * N);
    fclose(f);
    std::vector<float> col(3 * V * N), d_sh(N * W), d_xyz(3 * N);
    switch (deg) {
        case 0: run<0>(N, V, eval_mode, sh, xyz, cams, g, col, d_sh, d_xyz); break;
        case 1: run<1>(N, V, eval_mode, sh, xyz, cams, g, col, d_sh, d_xyz); break;
        case 2: run<2>(N, V, eval_mode, sh, xyz, cams, g, col, d_sh, d_xyz); break;
        case 3: run<3>(N, V, eval_mode, sh, xyz, cams, g, col, d_sh, d_xyz); break;
        case 4: run<4>(N, V, eval_mode, sh, xyz, cams, g, col, d_sh, d_xyz); break;
        default: return 5;
    }
    FILE* w = fopen(argv[2], "wb");
    if (!w) return 2;
    wr(w, col); wr(w, d_sh); wr(w, d_xyz);
    fclose(w);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("shcolor_math")
    src, exe = d / "harness.cpp", d / "harness"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", CSRC, str(src), "-o", str(exe)])

    def run(deg, sh, xyz, cams, g, eval_mode):
        N, V, W = sh.shape[0], cams.shape[0], 3 * (deg + 1) ** 2
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([deg, N, V, int(eval_mode)], np.int32).tobytes())
            for v in (sh[:, :(deg + 1) ** 2], xyz, cams, g):
                f.write(np.ascontiguousarray(v, R.F).tobytes())
        subprocess.check_call([str(exe), str(d / "in.bin"), str(d / "out.bin")])
        raw = np.fromfile(d / "out.bin", R.F)
        assert raw.size == 3 * V * N + N * W + 3 * N
        return raw[:3 * V * N].reshape(V, N, 3), raw[3 * V * N:3 * V * N + N * W].reshape(N, -1, 3), raw[3 * V * N + N * W:].reshape(N, 3)
    return run


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_row_arithmetic_of_the_kernels_equals_the_float32_statement_bit_for_bit(harness, deg):
    """csrc/shcolor_math.h is what the kernels compute per row; built here for the host, without contraction as build.py builds it
    for the device.  Random rows plus a point at the camera centre and a NaN coefficient; three views; both modes."""
    N, V, A = 3000, 3, (deg + 1) ** 2
    sh, xyz, cams, g = R.random_case(N, 25, seed=40 + deg, V=V)
    xyz[5] = cams[1]                    # 0 / 0 in view 1
    sh[9, 0, 1] = np.nan
    col, d_sh, d_xyz = harness(deg, sh, xyz, cams, g, False)
    want = R.S32.colors_views(deg, sh, xyz, cams)
    w_sh, w_xyz = R.S32.colors_backward(deg, sh, xyz, cams, g)
    assert R.same_class_and_bits(col, want)
    assert R.same_class_and_bits(d_sh, w_sh[:, :A]) and not w_sh[:, A:].any()
    assert R.same_class_and_bits(d_xyz, w_xyz)
    assert np.isnan(col[:, 9, 1]).all() and not np.isnan(np.delete(col[:, 9], 1, axis=1)).any()
    if deg:
        assert np.isnan(col[1, 5]).all() and not np.isnan(col[0, 5]).any() and (col == 0).mean() > 0.01 and d_xyz[:5].any()
    else:
        assert not np.isnan(col[:, 5]).any() and not d_xyz.any()
    # eval_sh: the directions as given (not unit length here: used as they are), no clamp
    dirs = (xyz / np.float32(3)).astype(R.F)
    col, d_sh, d_dirs = harness(deg, sh, dirs, cams[:1], g[:1], True)
    e_sh, e_dirs = R.S32.eval_sh_backward(deg, sh, dirs, g[0])
    assert R.same_class_and_bits(col[0], R.S32.eval_sh(deg, sh, dirs))
    assert R.same_class_and_bits(d_sh, e_sh[:, :A]) and R.same_class_and_bits(d_dirs, e_dirs)
    assert (col[0][~np.isnan(col[0])] < -0.5).any()


# ---- structure ----
def test_structs_match_c_layout(tmp_path):
    from texgs import shcolor
    consts = {"TEXGS_SH_COLORS_ROWS_PER_WORKGROUP": shcolor.ROWS_PER_WORKGROUP,
              "TEXGS_SH_COLORS_ROWS_PER_WORKGROUP_DEG4": shcolor.ROWS_PER_WORKGROUP_DEG4, "TEXGS_SH_COLORS_MAX_VIEWS": shcolor.MAX_VIEWS,
              "TEXGS_SH_COLORS_MAX_DEGREE": shcolor.MAX_DEGREE, "TEXGS_SH_COLORS": shcolor.MODE_COLORS, "TEXGS_SH_EVAL": shcolor.MODE_EVAL,
              "TEXGS_SH_LAYOUT_KC": shcolor.LAYOUT_KC, "TEXGS_SH_LAYOUT_CK": shcolor.LAYOUT_CK}
    assert sorted(shcolor.MIRRORS) == ["TexGSShColorGradView", "TexGSShColorView", "TexGSShColors", "TexGSShColorsGrad"]
    assert abi_check.layout_mismatches("texgs_shcolor.h", shcolor.MIRRORS, consts, tmp_path) == []
    assert C.sizeof(shcolor.ShColorViewStruct) == C.sizeof(shcolor.ShColorGradViewStruct) == 16


def test_header_compiles_as_c_and_as_cpp_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_shcolor.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "texgs_shcolor.h"\nint main(){return 0;}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "cpp.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert "TEXGS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "texgs_shcolor.h"' in open(os.path.join(CSRC, "shcolor.hip")).read()
    assert re.search(r"#define TEXGS_ABI_VERSION 19\b", open(os.path.join(INC, "texgs.h")).read())
    # the kernels: plain C++, no inline assembly, no atomics
    for name in ("shcolor.hip", "shcolor_math.h"):
        assert not re.search(r"\basm\b|__asm|atomic", open(os.path.join(CSRC, name)).read()), name


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib, shcolor
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(shcolor.SIGNATURES) == ["texgs_sh_colors_backward", "texgs_sh_colors_forward"]
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, shcolor.SIGNATURES, shcolor.MIRRORS) == []
    lib = shcolor.entry()
    assert lib is _lib.load() and lib.texgs_sh_colors_forward.argtypes == shcolor.SIGNATURES["texgs_sh_colors_forward"][1]
    assert lib.texgs_abi_version() == 19
    assert not any(n in _lib.SIGNATURES for n in protos)
    build = abi_check.build_knows_header(HDR)
    abi_check.build_knows_header(os.path.join(CSRC, "shcolor_math.h"))
    assert build.UNITS["shcolor.hip"] == ["-ffp-contract=off"]


def test_c_entries_refuse_bad_arguments_before_any_launch(lib_built):
    """No GPU here: a call that got as far as a launch would fail with a HIP error instead of the cause named below."""
    from texgs import shcolor as S
    lib = S.entry()
    buf = (C.c_double * 64)()            # stands in for every device buffer: nothing may read it
    b = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.texgs_last_error().decode()
    F = lambda **kw: S.ShColorsStruct(**{**dict(sh=b, sh_dc=None, sh_rest=None, xyz=b, n=5, coeffs=16, degree=3, layout=0, mode=0), **kw})
    views = lambda n=1, **kw: (S.ShColorViewStruct * n)(*[S.ShColorViewStruct(**{**dict(campos=b, colors=b), **kw}) for _ in range(n)])
    common = [
        (dict(degree=-1), 1, "degree must be in [0,4]"), (dict(degree=5, coeffs=25), 1, "degree must be in [0,4]"),
        (dict(coeffs=0), 1, "coeffs must be 1, 4, 9, 16 or 25"), (dict(coeffs=15), 1, "coeffs must be 1, 4, 9, 16 or 25"),
        (dict(coeffs=36, degree=4), 1, "coeffs must be 1, 4, 9, 16 or 25"), (dict(coeffs=9), 1, "(degree + 1)^2 exceeds coeffs"),
        (dict(coeffs=16, degree=4), 1, "(degree + 1)^2 exceeds coeffs"), (dict(n=-1), 1, "n < 0"),
        (dict(n=2 ** 31 // 48 + 1), 1, "below 2^31"), (dict(n=2 ** 31 - 1, coeffs=1, degree=0), 1, "below 2^31"),
        (dict(layout=2), 1, "layout must be"), (dict(mode=2), 1, "mode must be"),
        (dict(), 0, "count < 1"), (dict(), -3, "count < 1"), (dict(), S.MAX_VIEWS + 1, "TEXGS_SH_COLORS_MAX_VIEWS"),
        (dict(mode=1), 2, "exactly one view"),
        (dict(sh_dc=b), 1, "both sh and the pair"), (dict(sh_rest=b), 1, "both sh and the pair"),
        (dict(sh=None, sh_dc=b, sh_rest=b, layout=1), 1, "layout 0 only"),
        (dict(sh=None), 1, "NULL argument (sh"), (dict(sh=None, sh_dc=b), 1, "NULL argument (sh_rest"),
        (dict(sh=b + 2), 1, "4-byte aligned"), (dict(sh=None, sh_dc=b + 1, sh_rest=b), 1, "4-byte aligned"),
        (dict(sh=None, sh_dc=b, sh_rest=b + 3), 1, "4-byte aligned"),
        (dict(xyz=None), 1, "NULL argument (xyz"), (dict(xyz=b + 2), 1, "4-byte aligned"),
    ]
    for kw, count, cause in common:
        assert lib.texgs_sh_colors_forward(C.byref(F(**kw)), views(max(count, 1)), count, None) != 0, kw
        assert cause in err(), (kw, err())
    for vkw, cause in [(dict(colors=None), "NULL argument (a view's colors"), (dict(campos=None), "NULL argument (a view's campos"),
                       (dict(colors=b + 2), "4-byte aligned"), (dict(campos=b + 1), "4-byte aligned")]:
        assert lib.texgs_sh_colors_forward(C.byref(F()), views(2, **vkw), 2, None) != 0, vkw
        assert cause in err(), (vkw, err())
    assert lib.texgs_sh_colors_forward(None, views(), 1, None) != 0 and "NULL" in err()
    assert lib.texgs_sh_colors_forward(C.byref(F()), None, 1, None) != 0 and "NULL argument (views)" in err()
    # n = 0 launches nothing and accepts NULL data pointers; the shape is still checked
    assert lib.texgs_sh_colors_forward(C.byref(F(n=0, sh=None, xyz=None)), views(colors=None, campos=None), 1, None) == 0
    assert lib.texgs_sh_colors_forward(C.byref(F(n=0, degree=7)), views(), 1, None) != 0

    G = lambda **kw: S.ShColorsGradStruct(**{**dict(sh=b, sh_dc=None, sh_rest=None, xyz=b, d_sh=b, d_sh_dc=None, d_sh_rest=None, d_xyz=b,
                                                    n=5, coeffs=16, degree=3, layout=0, mode=0, accumulate=0), **kw})
    gviews = lambda n=1, **kw: (S.ShColorGradViewStruct * n)(*[S.ShColorGradViewStruct(**{**dict(campos=b, g_colors=b), **kw})
                                                               for _ in range(n)])
    for kw, count, cause in common + [
            (dict(accumulate=2), 1, "accumulate must be 0 or 1"), (dict(d_sh=None, d_xyz=None), 1, "no output requested"),
            (dict(sh=None, sh_dc=b, sh_rest=b), 1, "d_sh belongs to sh"), (dict(d_sh=None, d_sh_dc=b), 1, "belong to the pair"),
            (dict(d_sh=None, d_sh_rest=b), 1, "belong to the pair"), (dict(d_sh=b + 2), 1, "4-byte aligned"), (dict(d_xyz=b + 1), 1, "4-byte aligned"),
            (dict(sh=None, sh_dc=b, sh_rest=b, d_sh=None, d_sh_dc=b + 2), 1, "4-byte aligned")]:
        assert lib.texgs_sh_colors_backward(C.byref(G(**kw)), gviews(max(count, 1)), count, None) != 0, kw
        assert cause in err(), (kw, err())
    for vkw, cause in [(dict(g_colors=None), "NULL argument (a view's g_colors"), (dict(campos=None), "NULL argument (a view's campos"),
                       (dict(g_colors=b + 2), "4-byte aligned")]:
        assert lib.texgs_sh_colors_backward(C.byref(G()), gviews(3, **vkw), 3, None) != 0, vkw
        assert cause in err(), (vkw, err())
    assert lib.texgs_sh_colors_backward(None, gviews(), 1, None) != 0 and "NULL" in err()
    assert lib.texgs_sh_colors_backward(C.byref(G()), None, 1, None) != 0 and "NULL argument (views)" in err()
    assert lib.texgs_sh_colors_backward(C.byref(G(n=0, sh=None, xyz=None, d_sh=None, d_xyz=None)), gviews(g_colors=None), 1, None) == 0


# ---- texgs.shcolor refuses by name, before the "no CPU fallback" error ----
def test_every_validation_error_comes_before_the_cpu_refusal():
    from texgs import shcolor as S
    f, x, c = torch.zeros(5, 16, 3), torch.ones(5, 3), torch.zeros(3)
    dc, rest = torch.zeros(5, 1, 3), torch.zeros(5, 15, 3)
    col = lambda features=f, xyz=x, campos=c, degree=3: S.sh_colors(features, xyz, campos, degree)
    vws = lambda features=f, xyz=x, camposes=torch.zeros(2, 3), degree=3: S.sh_colors_views(features, xyz, camposes, degree)
    ev = lambda deg=3, sh=f.transpose(1, 2), dirs=x: S.eval_sh(deg, sh, dirs)
    meta = lambda *s: torch.zeros(*s, device="meta")
    bad = [
        (TypeError, "features must be a torch.Tensor", lambda: col(features=np.zeros((5, 16, 3), np.float32))),
        (ValueError, "features must be torch.float32", lambda: col(features=f.double())),
        (ValueError, r"features must be \[N,K,3\]", lambda: col(features=torch.zeros(5, 16))),
        (ValueError, r"features must be \[N,K,3\]", lambda: col(features=torch.zeros(5, 3, 16))),
        (ValueError, "features must be contiguous", lambda: col(features=torch.zeros(5, 32, 3)[:, ::2])),
        (ValueError, "features as a pair", lambda: col(features=(dc, rest, rest))),
        (TypeError, "features_dc must be a torch.Tensor", lambda: col(features=(None, rest))),
        (ValueError, r"features_dc must be \[N,1,3\]", lambda: col(features=(torch.zeros(5, 2, 3), rest))),
        (ValueError, r"features_rest must be \[N,K-1,3\]", lambda: col(features=(dc, torch.zeros(5, 15)))),
        (ValueError, "features_rest must be torch.float32", lambda: col(features=(dc, rest.half()))),
        (ValueError, "features_rest must be contiguous", lambda: col(features=(dc, torch.zeros(5, 30, 3)[:, ::2]))),
        (ValueError, "mismatched N", lambda: col(features=(dc, torch.zeros(4, 15, 3)))),
        (TypeError, "xyz must be a torch.Tensor", lambda: col(xyz=None)),
        (ValueError, r"xyz must be \[N,3\]", lambda: col(xyz=torch.zeros(5, 4))),
        (ValueError, "xyz must be torch.float32", lambda: col(xyz=x.double())),
        (ValueError, "xyz must be contiguous", lambda: col(xyz=torch.zeros(3, 5).t())),
        (ValueError, "mismatched N", lambda: col(xyz=torch.zeros(6, 3))),
        (TypeError, "campos must be a torch.Tensor", lambda: col(campos=[0.0, 0.0, 0.0])),
        (ValueError, r"campos must be \[3\] or \[1,3\]", lambda: col(campos=torch.zeros(2, 3))),
        (ValueError, "campos must be torch.float32", lambda: col(campos=c.double())),
        (ValueError, r"camposes must be \[V,3\]", lambda: vws(camposes=torch.zeros(3))),
        (ValueError, r"camposes must be \[V,3\]", lambda: vws(camposes=torch.zeros(0, 3))),
        (TypeError, "degree must be an int", lambda: col(degree=3.0)),
        (TypeError, "degree must be an int", lambda: col(degree=True)),
        (ValueError, r"degree must be in \[0, 4\]", lambda: col(degree=-1)),
        (ValueError, r"degree must be in \[0, 4\]", lambda: col(features=torch.zeros(5, 25, 3), degree=5)),
        (ValueError, "degree 4 needs 25 coefficients", lambda: col(degree=4)),
        (ValueError, "K must be one of", lambda: col(features=torch.zeros(5, 15, 3))),
        (ValueError, "K must be one of", lambda: col(features=(dc, torch.zeros(5, 14, 3)))),
        (ValueError, "campos is on meta", lambda: col(campos=meta(3))),
        (ValueError, "xyz is on meta", lambda: vws(xyz=meta(5, 3))),
        (TypeError, "sh must be a torch.Tensor", lambda: ev(sh=None)),
        (ValueError, r"sh must be \[N,3,K\]", lambda: ev(sh=f)),
        (ValueError, "sh must be torch.float32", lambda: ev(sh=f.transpose(1, 2).double())),
        (ValueError, r"dirs must be \[N,3\]", lambda: ev(dirs=torch.zeros(5))),
        (ValueError, "dirs must be contiguous", lambda: ev(dirs=torch.zeros(3, 5).t())),
        (ValueError, "mismatched N", lambda: ev(dirs=torch.zeros(4, 3))),
        (ValueError, "degree 4 needs 25 coefficients", lambda: ev(deg=4)),
        (ValueError, "taken without a copy", lambda: ev(sh=torch.zeros(5, 3, 32)[:, :, ::2])),
        (ValueError, "dirs is on meta", lambda: ev(dirs=meta(5, 3))),
    ]
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()
    # valid arguments on the CPU: refused as such, never computed in torch
    for call in (lambda: col(), lambda: col(features=(dc, rest)), lambda: col(campos=torch.zeros(1, 3), degree=0), lambda: vws(),
                 lambda: vws(camposes=torch.zeros(17, 3)), lambda: ev(), lambda: ev(sh=torch.zeros(5, 3, 16)), lambda: ev(deg=0),
                 lambda: col(features=torch.zeros(0, 25, 3), xyz=torch.zeros(0, 3), degree=4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
