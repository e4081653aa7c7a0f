"""-m "not gpu": the parameter stage (texgs/params.py, include/texgs_params.h, csrc/params_math.h) without a GPU.

* The float64 statement (tests/params_ref.py) against torch's own autograd in float64 on the CPU, values and all gradients, with the
  reference's composition written out here; the float32 statement's exp and log against float64.
* The kernels' row arithmetic (csrc/params_math.h) compiled for the host with g++ against the float32 statement, bit for bit.
* Structure: the ctypes mirrors against gcc's layout of the header's structs, the header as C and as C++, the exports and their
  signatures against the prototypes, the C entries' refusals (they need no GPU), the build script's knowledge of the unit.
* Every validation error of texgs.params is raised on CPU tensors BEFORE the "no CPU fallback" error."""
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
import params_ref as R  # noqa: E402
from texgs import params as _params  # noqa: E402,F401  (the feature under test: without it this file fails at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_params.h")
CSRC = os.path.join(ROOT, "texture-gs_amd", "csrc")
EPS = 1e-3


# ---- the statement ----
def _rows_with_small_norms(N, seed):
    scaling, rotation, opacity = R.random_rows(N, seed)
    rotation = rotation.astype(np.float64)
    rotation[3] = [3e-13, -2e-13, 1e-13, 0.0]         # below F.normalize's eps: the divisor is the constant
    rotation[7] = [0.0, 0.0, 0.0, 0.0]
    rotation[11] = [0.0, 5e-12, 0.0, 0.0]             # just above it
    return scaling.astype(np.float64), rotation, opacity.astype(np.float64)


def _torch_cov(scaling, rotation, modifier):
    """R S S^T R^T stripped in strip_lowerdiag's order, as utils/general.py composes it"""
    s = modifier * torch.exp(scaling)
    norm = torch.sqrt(rotation[:, 0] * rotation[:, 0] + rotation[:, 1] * rotation[:, 1] + rotation[:, 2] * rotation[:, 2]
                      + rotation[:, 3] * rotation[:, 3])
    q = rotation / norm[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = Rm @ torch.diag_embed(s)
    cov = L @ L.transpose(1, 2)
    return torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)


def test_float64_statement_equals_torch_autograd():
    """Values and every gradient to 1e-12 of each field's scale (an element's own magnitude; |g| / max(n, eps) per row for the
    gradient of rotation; the sum of the magnitudes of the two contributions for the gradient of opacity)"""
    from texgs import losses as LS
    N = 300
    a, q, x = _rows_with_small_norms(N, seed=3)
    g = {k: np.asarray(v, np.float64) for k, v in R.random_grads(N, seed=3).items()}
    ta, tq, tx = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (a, q, x))
    s, r, o = torch.exp(ta), torch.nn.functional.normalize(tq), torch.sigmoid(tx)
    reg = LS.zero_one_loss(o, EPS)
    loss = (s * torch.tensor(g["g_scales"])).sum() + (r * torch.tensor(g["g_rotations"])).sum() + (o * torch.tensor(g["g_opacities"])).sum() \
        + float(g["g_reg"]) * reg
    loss.backward()
    f = R.S64.activate(a, q, x, EPS)
    d = R.S64.activate_backward(q, f["scales"], f["opacities"], g["g_scales"], g["g_rotations"], g["g_opacities"], g["g_reg"], EPS)
    tol = 1e-12
    assert R.max_error(f["scales"], s.detach().numpy(), np.abs(f["scales"])) <= tol
    assert R.max_error(f["rotations"], r.detach().numpy(), np.maximum(np.abs(f["rotations"]), 1e-300)) <= tol
    assert R.max_error(f["opacities"], o.detach().numpy().reshape(-1), f["opacities"]) <= tol
    assert abs(float(f["reg"]) - float(reg.detach())) <= tol * abs(float(reg.detach()))
    assert R.max_error(d[0], ta.grad.numpy(), np.abs(d[0])) <= tol
    n = np.maximum(f["norm"], 1e-12)
    assert R.max_error(d[1], tq.grad.numpy(), (np.linalg.norm(g["g_rotations"], axis=1) / n)[:, None]) <= tol
    assert np.abs(d[1][3]).max() > 1e11 and np.array_equal(d[1][7], g["g_rotations"][7] / 1e-12)          # the rows below eps
    oo = f["opacities"]
    v = np.clip(oo, EPS, 1 - EPS)
    scale = (np.abs(g["g_opacities"].reshape(-1)) + np.abs(g["g_reg"] / N * (1 / v - 1 / (1 - v)))) * oo * (1 - oo)
    assert R.max_error(d[2], tx.grad.numpy().reshape(-1), scale) <= tol
    assert ((oo < EPS) | (oo > 1 - EPS)).sum() > 20           # the clamp is exercised on both sides of its edges
    # the regulariser alone, and each upstream gradient absent in turn
    for drop in ("g_scales", "g_rotations", "g_opacities", "g_reg"):
        kw = {k: (None if k == drop else g[k]) for k in ("g_scales", "g_rotations", "g_opacities", "g_reg")}
        kz = {k: (np.zeros_like(g[k]) if k == drop else g[k]) for k in kw}
        got = R.S64.activate_backward(q, f["scales"], f["opacities"], epsilon=EPS, **kw)
        want = R.S64.activate_backward(q, f["scales"], f["opacities"], epsilon=EPS, **kz)
        assert all(np.array_equal(u, w) for u, w in zip(got, want)), drop
    # the covariance (no zero quaternion: build_rotation divides by the norm)
    a, q, _ = (v.astype(np.float64) for v in R.random_rows(N, seed=4))
    for modifier in (1.0, 0.37):
        ta, tq = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (a, q))
        cov = _torch_cov(ta, tq, modifier)
        (cov * torch.tensor(g["g_cov"])).sum().backward()
        got = R.S64.covariance(a, q, modifier)
        s2 = ((modifier * np.exp(a)).max(axis=1) ** 2)[:, None]
        assert R.max_error(got, cov.detach().numpy(), s2) <= tol
        da, dq = R.S64.covariance_backward(a, q, modifier, g["g_cov"])
        assert R.max_error(da, ta.grad.numpy(), s2) <= tol
        assert R.max_error(dq, tq.grad.numpy(), s2 / np.linalg.norm(q, axis=1)[:, None]) <= tol
    assert not np.isfinite(R.S64.covariance(a[:1], np.zeros((1, 4)), 1.0)).any()           # documented, not checked


def test_float32_exp_and_log_are_within_one_ulp_and_have_the_stated_edges():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-87.0, 88.0, 200000), rng.uniform(-1.0, 1.0, 50000), np.linspace(-104.0, -87.0, 5000)]).astype(R.F)
    got = R.exp32(x).astype(np.float64)
    want = np.exp(x.astype(np.float64))
    ulp = np.maximum(np.spacing(want.astype(R.F)).astype(np.float64), 2.0 ** -149)
    err = np.abs(got - want) / ulp
    print("exp32: largest error in ulp", err.max())
    assert err.max() <= 1.0
    e = R.exp32(np.array([89.0, 88.8, -104.0, -110.5, -1e30, 1e30, np.inf, -np.inf, 0.0, np.nan], R.F))
    assert np.isinf(e[0]) and np.isinf(e[1]) and e[2] == 0 and e[3] == 0 and e[4] == 0 and np.isinf(e[5]) and np.isinf(e[6]) and e[7] == 0
    assert e[8] == 1 and np.isnan(e[9])
    assert R.exp32(np.array([88.7], R.F))[0] < np.inf and R.exp32(np.array([-103.0], R.F))[0] > 0           # subnormal, not flushed
    v = np.concatenate([rng.uniform(1e-6, 1.0, 200000), 1.0 - 10.0 ** rng.uniform(-7, -1, 50000), 10.0 ** rng.uniform(-38, 38, 50000)]).astype(R.F)
    v = v[v > 0]
    got = R.log32(v).astype(np.float64)
    want = np.log(v.astype(np.float64))
    err = np.abs(got - want) / np.maximum(np.spacing(np.abs(want).astype(R.F)).astype(np.float64), 2.0 ** -149)
    print("log32: largest error in ulp", err.max())
    assert err.max() <= 1.0
    # sigmoid: monotone enough for the bisection of edge_logits, and its edges
    o = R.S32.sigmoid(np.array([17.0, -17.0, 90.0, -90.0, 0.0], R.F))
    assert o[0] == 1 and 0 < o[1] < 1e-7 and o[2] == 1 and o[3] == 0 and o[4] == 0.5
    edges = R.edge_logits(EPS)
    oe = R.S32.sigmoid(edges)
    # a float32 step of the logit moves the sigmoid by several units in its last place there, so epsilon itself is not reached
    # through the forward: the logits straddle each edge, and the edges themselves are fed to the backward as opacities
    lo, hi = R.F(EPS), R.F(1) - R.F(EPS)
    assert (oe < lo).any() and (oe >= lo).any() and (oe <= hi).any() and (oe > hi).any()
    assert np.abs(oe.astype(np.float64) - lo).min() < 1e-9 and (oe == hi).any()
    o = R.edge_opacities(EPS)
    assert (o == lo).any() and (o == hi).any() and o.size == 6
    for S, t in ((R.S64, torch.float64), (R.S32, torch.float32)):
        d = S.activate_backward(np.ones((6, 4)), np.ones((6, 3)), o, g_reg=1.0, epsilon=EPS)[2]
        to = torch.tensor(o.astype(S.T), requires_grad=True)
        v = torch.clamp(to, float(S.T(EPS)), float(S.T(1) - S.T(EPS)))              # the statement's own edges, as torch sees them
        torch.mean(torch.log(v) + torch.log(1 - v)).backward()
        assert np.array_equal(d != 0, to.grad.numpy() != 0), S.T
    assert np.array_equal(R.S32.activate_backward(np.ones((6, 4)), np.ones((6, 3)), o, g_reg=1.0, epsilon=EPS)[2] != 0,
                          [False, True, True, True, True, False])


HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "params_math.h"
namespace pm = params_math;
static std::vector<float> rd(FILE* f, size_t n) { std::vector<float> v(n); if (n && fread(v.data(), 4, n, f) != n) exit(3); return v; }
static void wr(FILE* f, const std::vector<float>& v) { if (v.size() && fwrite(v.data(), 4, v.size(), f) != v.size()) exit(4); }
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n; float head[3];
    if (fread(&n, 4, 1, f) != 1 || fread(head, 4, 3, f) != 3) return 3;
    const float eps = head[0], m = head[1], g_reg = head[2];
    const size_t N = (size_t)n;
    auto a = rd(f, 3 * N), q = rd(f, 4 * N), x = rd(f, N), gs = rd(f, 3 * N), gr = rd(f, 4 * N), go = rd(f, N), gc = rd(f, 6 * N);
    fclose(f);
    std::vector<float> s(3 * N), r(4 * N), o(N), term(N), ds(3 * N), dr(4 * N), dop(N), cov(6 * N), cda(3 * N), cdq(4 * N);
    const float c = g_reg / (float)(unsigned)n;
    for (size_t i = 0; i < N; ++i) {
        for (int k = 0; k < 3; ++k) s[3 * i + k] = pm::exp32(a[3 * i + k]);
        pm::normalize(&q[4 * i], &r[4 * i]);
        o[i] = pm::sigmoid32(x[i]);
        term[i] = pm::reg_term(o[i], eps);
        for (int k = 0; k < 3; ++k) ds[3 * i + k] = gs[3 * i + k] * s[3 * i + k];
        pm::normalize_backward(&q[4 * i], &gr[4 * i], &dr[4 * i]);
        dop[i] = pm::opacity_backward(o[i], go[i], true, c, eps);
        pm::covariance(&a[3 * i], &q[4 * i], m, &cov[6 * i]);
        pm::covariance_backward(&a[3 * i], &q[4 * i], m, &gc[6 * i], &cda[3 * i], &cdq[4 * i]);
    }
    FILE* w = fopen(argv[2], "wb");
    if (!w) return 2;
    wr(w, s); wr(w, r); wr(w, o); wr(w, term); wr(w, ds); wr(w, dr); wr(w, dop); wr(w, cov); wr(w, cda); wr(w, cdq);
    fclose(w);
    return 0;
}
"""


def test_row_arithmetic_of_the_kernels_equals_the_float32_statement_bit_for_bit(tmp_path):
    """csrc/params_math.h is what the kernels compute per row; built here for the host, without contraction as build.py builds it
    for the device.  Random rows and the special rows, every field, forward and backward.  (Rows whose covariance is not finite are
    compared by class: a NaN's payload is not part of the contract.)"""
    src, exe = tmp_path / "harness.cpp", tmp_path / "harness"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    a1, q1, x1 = R.random_rows(4000, seed=5)
    a2, q2, x2 = R.special_rows(EPS)
    a, q, x = np.concatenate([a1, a2]), np.concatenate([q1, q2]), np.concatenate([x1, x2])
    N = a.shape[0]
    g = R.random_grads(N, seed=5)
    m = R.F(0.37)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(N).tobytes() + np.array([EPS, m, g["g_reg"]], R.F).tobytes())
        for v in (a, q, x, g["g_scales"], g["g_rotations"], g["g_opacities"], g["g_cov"]):
            f.write(np.ascontiguousarray(v, R.F).tobytes())
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = np.fromfile(tmp_path / "out.bin", R.F)
    widths = dict(scales=3, rotations=4, opacities=1, terms=1, d_scaling=3, d_rotation=4, d_opacity=1, cov=6, cov_d_scaling=3, cov_d_rotation=4)
    assert raw.size == N * sum(widths.values())
    got, at = {}, 0
    for k, w in widths.items():
        got[k] = raw[at:at + N * w].reshape(N, w)
        at += N * w
    f32 = R.S32.activate(a, q, x, EPS)
    b = R.S32.activate_backward(q, f32["scales"], f32["opacities"], g["g_scales"], g["g_rotations"], g["g_opacities"], g["g_reg"], EPS)
    cb = R.S32.covariance_backward(a, q, m, g["g_cov"])
    want = dict(scales=f32["scales"], rotations=f32["rotations"], opacities=f32["opacities"], terms=f32["terms"], d_scaling=b[0], d_rotation=b[1],
                d_opacity=b[2], cov=R.S32.covariance(a, q, m), cov_d_scaling=cb[0], cov_d_rotation=cb[1])
    for k in widths:
        assert R.same_class_and_bits(got[k], want[k].reshape(N, -1)), k
    # the special rows are special: an overflow, an underflow to zero, a zero row, a row of q / 1e-12, a non-finite covariance
    sp = slice(N - a2.shape[0], N)
    assert np.isinf(got["scales"][sp]).any() and (got["scales"][sp] == 0).any()
    assert (got["rotations"][sp][2] == 0).all() and np.array_equal(got["rotations"][sp][1], np.full(4, R.F(1e-25) / R.F(1e-12), R.F))
    assert not np.isfinite(got["cov"][sp][0]).any()


# ---- structure ----
def test_structs_match_c_layout(tmp_path):
    from texgs import params
    consts = {"TEXGS_PARAMS_ROWS_PER_WORKGROUP": params.ROWS_PER_WORKGROUP}
    assert sorted(params.MIRRORS) == ["TexGSParamsActivate", "TexGSParamsActivateGrad", "TexGSParamsCovariance", "TexGSParamsCovarianceGrad"]
    assert abi_check.layout_mismatches("texgs_params.h", params.MIRRORS, consts, tmp_path) == []


def test_header_compiles_as_c_and_as_cpp_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_params.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "texgs_params.h"\nint main(){return 0;}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(cpp), "-o", str(tmp_path / "cpp.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert "TEXGS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "texgs_params.h"' in open(os.path.join(CSRC, "params.hip")).read()
    assert re.search(r"#define TEXGS_ABI_VERSION 19\b", open(os.path.join(INC, "texgs.h")).read())
    # the kernels: plain C++, no inline assembly
    for name in ("params.hip", "params_math.h"):
        assert not re.search(r"\basm\b|__asm", open(os.path.join(CSRC, name)).read()), name


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib, params
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(params.SIGNATURES) == sorted(
        ["texgs_params_temp_bytes", "texgs_params_activate", "texgs_params_activate_backward", "texgs_params_covariance",
         "texgs_params_covariance_backward"])
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, params.SIGNATURES, params.MIRRORS) == []
    lib = params.entry()
    assert lib is _lib.load() and lib.texgs_params_activate.argtypes == params.SIGNATURES["texgs_params_activate"][1]
    assert lib.texgs_abi_version() == 19
    assert not any(n in _lib.SIGNATURES for n in protos) and not hasattr(_lib, "ParamsActivateStruct")
    build = abi_check.build_knows_header(HDR)
    assert build.UNITS["params.hip"] == ["-ffp-contract=off"]


def test_c_entries_refuse_bad_arguments_before_any_launch(lib_built):
    """No GPU here: a call that got as far as a launch would fail with a HIP error instead of the cause named below."""
    from texgs import params
    lib = params.entry()
    buf = (C.c_double * 64)()            # stands in for every device buffer: nothing may read it
    b = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.texgs_last_error().decode()
    RPW = params.ROWS_PER_WORKGROUP
    tb = lib.texgs_params_temp_bytes
    assert tb(0) == 0 and tb(-5) == 0 and tb(1) == 256 and tb(32 * RPW) == 256 and tb(32 * RPW + 1) == 512
    assert tb(2 ** 31 - 1) == (8 * (2 ** 31 // RPW) + 255) // 256 * 256
    nan, inf = float("nan"), float("inf")

    A = lambda **kw: params.ParamsActivateStruct(**{**dict(scaling=b, rotation=b, opacity=b, scales=b, rotations=b, opacities=b, reg=b,
                                                           epsilon=1e-3, n=5), **kw})
    for kw, temp, nbytes, cause in [
            (dict(n=-1), b, 256, "n < 0"),
            (dict(scales=None, rotations=None, opacities=None, reg=None), b, 256, "no output requested"),
            (dict(scaling=None), b, 256, "NULL argument"), (dict(rotation=None), b, 256, "NULL argument"),
            (dict(opacity=None), b, 256, "NULL argument"), (dict(opacity=None, opacities=None), b, 256, "NULL argument"),
            (dict(), None, 256, "NULL argument (temp"),
            (dict(epsilon=0.0), b, 256, "epsilon must lie in (0, 0.5)"), (dict(epsilon=0.5), b, 256, "epsilon must lie in (0, 0.5)"),
            (dict(epsilon=-1e-3), b, 256, "epsilon must lie in (0, 0.5)"), (dict(epsilon=nan), b, 256, "epsilon must lie in (0, 0.5)"),
            (dict(n=0), b, 256, "a mean over nothing"),
            (dict(), b, 255, "temp is smaller"), (dict(n=32 * RPW + 1), b, 256, "temp is smaller"),
            (dict(scaling=b + 2), b, 256, "4-byte aligned"), (dict(opacities=b + 1), b, 256, "4-byte aligned"), (dict(reg=b + 2), b, 256, "4-byte aligned"),
            (dict(rotation=b + 4), b, 256, "16-byte aligned"), (dict(rotations=b + 8), b, 256, "16-byte aligned"),
            (dict(), b + 4, 256, "temp must be 8-byte aligned")]:
        assert lib.texgs_params_activate(C.byref(A(**kw)), temp, nbytes, None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_params_activate(None, b, 256, None) != 0 and "NULL" in err()
    # n = 0 launches nothing and accepts NULL pointers; an unwanted output's input may be NULL (refused for another cause here)
    assert lib.texgs_params_activate(C.byref(params.ParamsActivateStruct(n=0)), None, 0, None) == 0
    assert lib.texgs_params_activate(C.byref(A(scaling=None, scales=None, rotation=None, rotations=None)), b, 255, None) != 0 and "temp is smaller" in err()

    G = lambda **kw: params.ParamsActivateGradStruct(**{**dict(scales=b, rotation=b, opacities=b, g_scales=b, g_rotations=b, g_opacities=b,
                                                               g_reg=b, d_scaling=b, d_rotation=b, d_opacity=b, epsilon=1e-3, n=5), **kw})
    for kw, cause in [
            (dict(n=-1), "n < 0"), (dict(d_scaling=None, d_rotation=None, d_opacity=None), "no output requested"),
            (dict(scales=None), "NULL argument"), (dict(rotation=None), "NULL argument"), (dict(opacities=None), "NULL argument"),
            (dict(opacities=None, g_opacities=None), "NULL argument"),
            (dict(epsilon=0.0), "epsilon must lie in (0, 0.5)"), (dict(epsilon=0.75), "epsilon must lie in (0, 0.5)"),
            (dict(epsilon=nan), "epsilon must lie in (0, 0.5)"),
            (dict(g_scales=b + 2), "4-byte aligned"), (dict(d_opacity=b + 3), "4-byte aligned"), (dict(g_reg=b + 1), "4-byte aligned"),
            (dict(g_rotations=b + 4), "16-byte aligned"), (dict(d_rotation=b + 8), "16-byte aligned"), (dict(rotation=b + 12), "16-byte aligned")]:
        assert lib.texgs_params_activate_backward(C.byref(G(**kw)), None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_params_activate_backward(None, None) != 0 and "NULL" in err()
    assert lib.texgs_params_activate_backward(C.byref(params.ParamsActivateGradStruct(n=0)), None) == 0

    V = lambda **kw: params.ParamsCovarianceStruct(**{**dict(scaling=b, rotation=b, cov=b, scale_modifier=1.0, n=5), **kw})
    for kw, cause in [(dict(n=-1), "n < 0"), (dict(scaling=None), "NULL argument"), (dict(rotation=None), "NULL argument"),
                      (dict(cov=None), "NULL argument"), (dict(scale_modifier=0.0), "finite and positive"),
                      (dict(scale_modifier=-1.0), "finite and positive"), (dict(scale_modifier=inf), "finite and positive"),
                      (dict(scale_modifier=nan), "finite and positive"), (dict(cov=b + 2), "4-byte aligned"), (dict(rotation=b + 4), "16-byte aligned")]:
        assert lib.texgs_params_covariance(C.byref(V(**kw)), None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_params_covariance(None, None) != 0 and "NULL" in err()
    assert lib.texgs_params_covariance(C.byref(params.ParamsCovarianceStruct(n=0, scale_modifier=1.0)), None) == 0

    W = lambda **kw: params.ParamsCovarianceGradStruct(**{**dict(scaling=b, rotation=b, g_cov=b, d_scaling=b, d_rotation=b, scale_modifier=1.0,
                                                                 n=5), **kw})
    for kw, cause in [(dict(n=-1), "n < 0"), (dict(scaling=None), "NULL argument"), (dict(rotation=None), "NULL argument"),
                      (dict(d_scaling=None, d_rotation=None), "no output requested"), (dict(scale_modifier=0.0), "finite and positive"),
                      (dict(scale_modifier=nan), "finite and positive"), (dict(scale_modifier=inf), "finite and positive"),
                      (dict(g_cov=b + 1), "4-byte aligned"), (dict(d_rotation=b + 4), "16-byte aligned")]:
        assert lib.texgs_params_covariance_backward(C.byref(W(**kw)), None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_params_covariance_backward(None, None) != 0 and "NULL" in err()
    assert lib.texgs_params_covariance_backward(C.byref(params.ParamsCovarianceGradStruct(n=0, scale_modifier=1.0)), None) == 0


# ---- texgs.params refuses by name, before the "no CPU fallback" error ----
def test_every_validation_error_comes_before_the_cpu_refusal():
    from texgs import params as P
    a, q, x = torch.zeros(5, 3), torch.ones(5, 4), torch.zeros(5, 1)
    act = lambda scaling=a, rotation=q, opacity=x, **kw: P.activate(scaling, rotation, opacity, **kw)
    cov = lambda scaling=a, rotation=q, **kw: P.covariance(scaling, rotation, **kw)
    meta = lambda *s: torch.zeros(*s, device="meta")
    bad = [
        (TypeError, "scaling must be a torch.Tensor", lambda: act(scaling=np.zeros((5, 3), np.float32))),
        (TypeError, "rotation must be a torch.Tensor", lambda: act(rotation=None)),
        (TypeError, "opacity must be a torch.Tensor", lambda: act(opacity=[0.0] * 5)),
        (ValueError, "scaling must be torch.float32", lambda: act(scaling=a.double())),
        (ValueError, "rotation must be torch.float32", lambda: act(rotation=q.half())),
        (ValueError, "opacity must be torch.float32", lambda: act(opacity=x.double())),
        (ValueError, r"scaling must be \[N,3\]", lambda: act(scaling=torch.zeros(5, 4))),
        (ValueError, r"scaling must be \[N,3\]", lambda: act(scaling=torch.zeros(15))),
        (ValueError, r"rotation must be \[N,4\]", lambda: act(rotation=torch.zeros(5, 3))),
        (ValueError, r"opacity must be \[N,1\] or \[N\]", lambda: act(opacity=torch.zeros(5, 2))),
        (ValueError, r"opacity must be \[N,1\] or \[N\]", lambda: act(opacity=torch.zeros(5, 1, 1))),
        (ValueError, "scaling must be contiguous", lambda: act(scaling=torch.zeros(3, 5).t())),
        (ValueError, "rotation must be contiguous", lambda: act(rotation=torch.zeros(5, 8)[:, ::2])),
        (ValueError, "opacity must be contiguous", lambda: act(opacity=torch.zeros(10)[::2])),
        (ValueError, "mismatched N", lambda: act(scaling=torch.zeros(4, 3))),
        (ValueError, "mismatched N", lambda: act(opacity=torch.zeros(6))),
        (TypeError, "opacity_reg must be a bool", lambda: act(opacity_reg=1)),
        (TypeError, "epsilon must be a number", lambda: act(epsilon="1e-3")),
        (ValueError, r"epsilon must lie in \(0, 0.5\)", lambda: act(epsilon=0.0)),
        (ValueError, r"epsilon must lie in \(0, 0.5\)", lambda: act(epsilon=0.5)),
        (ValueError, r"epsilon must lie in \(0, 0.5\)", lambda: act(epsilon=float("nan"))),
        (ValueError, r"epsilon must lie in \(0, 0.5\)", lambda: act(epsilon=1e-60)),             # zero as a float32
        (ValueError, "a mean over nothing", lambda: act(torch.zeros(0, 3), torch.zeros(0, 4), torch.zeros(0, 1), opacity_reg=True)),
        (ValueError, "rotation is on meta", lambda: act(rotation=meta(5, 4))),
        (TypeError, "opacity_param must be a torch.Tensor", lambda: P.zero_one_loss(3.0)),
        (ValueError, r"opacity_param must be \[N,1\] or \[N\]", lambda: P.zero_one_loss(torch.zeros(5, 3))),
        (ValueError, "opacity_param must be torch.float32", lambda: P.zero_one_loss(x.double())),
        (ValueError, r"epsilon must lie in \(0, 0.5\)", lambda: P.zero_one_loss(x, epsilon=0.6)),
        (ValueError, "a mean over nothing", lambda: P.zero_one_loss(torch.zeros(0))),
        (TypeError, "scaling must be a torch.Tensor", lambda: cov(scaling=None)),
        (ValueError, r"rotation must be \[N,4\]", lambda: cov(rotation=torch.zeros(5, 3))),
        (ValueError, "rotation must be torch.float32", lambda: cov(rotation=q.double())),
        (ValueError, "mismatched N", lambda: cov(rotation=torch.ones(6, 4))),
        (TypeError, "scale_modifier must be a number", lambda: cov(scale_modifier=torch.tensor(1.0))),
        (ValueError, "scale_modifier must be finite and positive", lambda: cov(scale_modifier=0.0)),
        (ValueError, "scale_modifier must be finite and positive", lambda: cov(scale_modifier=-2.0)),
        (ValueError, "scale_modifier must be finite and positive", lambda: cov(scale_modifier=float("inf"))),
        (ValueError, "scale_modifier must be finite and positive", lambda: cov(scale_modifier=float("nan"))),
        (ValueError, "scale_modifier must be finite and positive", lambda: cov(scale_modifier=1e39)),            # inf as a float32
        (ValueError, "scaling is on cpu, rotation is on meta|rotation is on meta", lambda: cov(rotation=meta(5, 4))),
    ]
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()
    # valid arguments on the CPU: refused as such, never computed in torch
    for call in (lambda: act(), lambda: act(opacity=torch.zeros(5), opacity_reg=True, epsilon=0.01), lambda: P.zero_one_loss(x),
                 lambda: P.zero_one_loss(torch.zeros(5)), lambda: cov(), lambda: cov(scale_modifier=2),
                 lambda: act(torch.zeros(0, 3), torch.zeros(0, 4), torch.zeros(0, 1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # texgs.losses.zero_one_loss stays plain torch
    from texgs import losses as LS
    assert float(LS.zero_one_loss(torch.full((4,), 0.5))) == pytest.approx(2 * np.log(0.5))
