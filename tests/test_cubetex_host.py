"""-m "not gpu": the float64 statement of seamless cubemap sampling (tests/cubetex_ref.py) against the pinned cube convention and
its own continuity across every edge and corner, latlong_dirs, the argument checks of texgs.cubetex, the nvdiffrast drop-in and
the additions to the C ABI."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubetex_ref as O  # noqa: E402

ENTRY_POINTS = ("texgs_cube_sample", "texgs_cube_latlong", "texgs_cube_sample_backward")


@pytest.mark.parametrize("filter", ["nearest", "linear"])
def test_oracle_returns_each_texel_at_its_centre(filter):
    d = np.load(os.path.join(ROOT, "tests", "golden", "cube.npz"))
    dirs = torch.tensor(d["dirs"])                   # [6, R, R, 3] at texel centres, util.cube_to_dir
    R = int(d["R"])
    tex = torch.arange(6 * R * R * 3, dtype=torch.float64).reshape(6, R, R, 3)
    got = O.sample(tex, (dirs * 2.5).reshape(-1, 3), filter).reshape(6, R, R, 3)     # any length
    assert torch.equal(got, tex)
    c = torch.tensor((np.arange(R) + 0.5) * 2 / R - 1)
    face = torch.arange(6)[:, None, None].expand(6, R, R)
    assert torch.equal(O.cube_to_dir(face, c[None, None, :].expand(6, R, R), c[None, :, None].expand(6, R, R)), dirs)


def _edges_and_corners():
    """12 edges and 8 corners of the cube [-1, 1]^3 as (point on it, the two or three outward axes-with-sign that meet there)"""
    edges, corners = [], []
    for a in range(3):
        for b in range(a + 1, 3):
            c = 3 - a - b
            for sa in (-1.0, 1.0):
                for sb in (-1.0, 1.0):
                    for along in (-0.83, -0.31, 0.0, 0.47, 0.9):
                        p = [0.0, 0.0, 0.0]
                        p[a], p[b], p[c] = sa, sb, along
                        edges.append((p, [(a, sa), (b, sb)]))
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                corners.append(([sx, sy, sz], [(0, sx), (1, sy), (2, sz)]))
    return edges, corners


@pytest.mark.parametrize("R", [4, 5])
def test_oracle_is_continuous_across_every_edge_and_corner(R):
    """A point on an edge (corner) of the cube, pushed 1e-9 outwards along each of the two (three) axes that meet there, lands on
    each of the faces in turn; the linear fetch must agree on them to 1e-7.  The texture is random, so a wrong neighbour, a
    reversed index or a corner weight that is not renormalised shows as a difference of order 1."""
    g = torch.Generator().manual_seed(R)
    tex = torch.rand(6, R, R, 2, generator=g, dtype=torch.float64)
    edges, corners = _edges_and_corners()
    assert len(edges) == 12 * 5 and len(corners) == 8
    for p, axes in edges + corners:
        vals, faces = [], []
        for axis, sign in axes:
            q = torch.tensor([p], dtype=torch.float64)
            q[0, axis] += sign * 1e-9
            faces.append(int(O.address(q, R)[0]))
            vals.append(O.sample(tex, q))
        assert len(set(faces)) == len(axes), (p, faces)              # really one value per face that meets there
        for v in vals[1:]:
            assert float((v - vals[0]).abs().max()) <= 1e-7, (p, faces)


@pytest.mark.parametrize("res", [(8, 16), (6, 10)])
def test_latlong_dirs_against_float64_restatement(res):
    """texgs.cubetex.latlong_dirs computes in float64 and rounds once, so it is within half an fp32 ulp of the float64 statement:
    every component is <= 1 in magnitude, so 2^-24 absolute; 4 ulp = 2^-21 is asserted.  The restatement here is written from the
    formula, index by index, with the poles' neighbours (first and last row) and the +-pi columns (first and last) included."""
    from texgs import cubetex
    H, W = res
    got = cubetex.latlong_dirs(res, "cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == (H, W, 3)
    want = torch.empty(H, W, 3, dtype=torch.float64)
    for i in range(H):
        gy = 1.0 / H + i * ((1.0 - 2.0 / H) / (H - 1))
        for j in range(W):
            gx = -1.0 + 1.0 / W + j * ((2.0 - 2.0 / W) / (W - 1))
            th, ph = math.pi * gy, math.pi * gx
            want[i, j] = torch.tensor([math.sin(th) * math.sin(ph), math.cos(th), -math.sin(th) * math.cos(ph)], dtype=torch.float64)
    assert torch.allclose(want, O.latlong_dirs(res), rtol=0, atol=1e-14)         # float64 against float64
    err = float((got.double() - want).abs().max())
    print(res, "latlong_dirs max abs error:", err)
    assert err <= 2.0 ** -21
    # first row looks near +y, last near -y; the first and last columns look near -z from either side (phi = -+pi)
    assert float(want[0, :, 1].min()) > 0.8 and float(want[-1, :, 1].max()) < -0.8
    assert float(got[H // 2, 0, 2]) > 0 and float(got[H // 2, -1, 2]) > 0
    assert float(got[H // 2, 0, 0]) < 0 < float(got[H // 2, -1, 0])


def test_arguments_are_checked_before_any_launch(lib_built, monkeypatch):
    from texgs import _lib, cubetex

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    tex = torch.rand(6, 4, 4, 3)
    dirs = torch.rand(7, 3)
    with pytest.raises(RuntimeError, match="texture must be on an AMD GPU; there is no CPU fallback"):
        cubetex.cube_sample(tex, dirs)
    for f in (lambda t: cubetex.cube_sample(t, dirs), lambda t: cubetex.cubemap_to_latlong(t, (4, 8)),
              lambda t: cubetex.sphere_map(t, (4, 8)), lambda t: cubetex.sphere_map(t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(tex)
        with pytest.raises(TypeError, match="texture must be a torch.Tensor"):
            f(tex.numpy())
        with pytest.raises(ValueError, match="texture must be float32"):
            f(tex.double())
        with pytest.raises(ValueError, match=r"texture must be \[6, R, R, C\]"):
            f(tex[0])
        with pytest.raises(ValueError, match=r"texture must be \[6, R, R, C\]"):
            f(torch.rand(5, 4, 4, 3))
        with pytest.raises(ValueError, match="faces must be square"):
            f(torch.rand(6, 4, 5, 3))
        with pytest.raises(ValueError, match="R >= 2"):
            f(torch.rand(6, 1, 1, 3))
        with pytest.raises(ValueError, match="C >= 1"):
            f(torch.rand(6, 4, 4, 0))
        with pytest.raises(ValueError, match="31 bits"):
            f(torch.empty(1).expand(6, 18920, 18920, 1))          # 6 * 18920^2 > 2^31, no memory behind it
    with pytest.raises(TypeError, match="dirs must be a torch.Tensor"):
        cubetex.cube_sample(tex, dirs.numpy())
    with pytest.raises(ValueError, match="dirs must be float32"):
        cubetex.cube_sample(tex, dirs.double())
    with pytest.raises(ValueError, match=r"dirs must be \[\.\.\., 3\]"):
        cubetex.cube_sample(tex, torch.rand(7, 2))
    with pytest.raises(ValueError, match=r"dirs must be \[\.\.\., 3\]"):
        cubetex.cube_sample(tex, torch.tensor(1.0))
    with pytest.raises(ValueError, match="filter must be 'linear' or 'nearest'"):
        cubetex.cube_sample(tex, dirs, "cubic")
    for bad in ((4,), (4, 0), (4, 8.0), 8, (True, 4), (2 ** 16, 2 ** 15)):
        with pytest.raises(ValueError, match="resolution"):
            cubetex.cubemap_to_latlong(tex, bad)
        with pytest.raises(ValueError, match="resolution"):
            cubetex.latlong_dirs(bad, "cpu")
    with pytest.raises(RuntimeError, match="dirs must be on an AMD GPU; there is no CPU fallback"):
        cubetex.chessboard_texture(dirs)
    with pytest.raises(ValueError, match=r"dirs must be \[\.\.\., 3\]"):
        cubetex.chessboard_texture(torch.rand(7, 2))
    with pytest.raises(ValueError, match="resolution must be a positive int"):
        cubetex.chessboard_texture(dirs, 0)


def test_c_entry_points_refuse_bad_sizes(lib_built):
    """The C layer's own checks return an error code before any launch (no GPU is needed to see them)."""
    from texgs import _lib
    lib = _lib.load()
    assert lib.texgs_cube_sample(None, 1, 3, None, 4, 0, 0, None, None) != 0
    assert b"R < 2" in lib.texgs_last_error()
    assert lib.texgs_cube_sample(None, 4, 0, None, 4, 0, 0, None, None) != 0
    assert b"C < 1" in lib.texgs_last_error()
    assert lib.texgs_cube_sample(None, 18920, 1, None, 4, 0, 0, None, None) != 0
    assert b"2^31" in lib.texgs_last_error()
    assert lib.texgs_cube_sample(None, 4, 3, None, -1, 0, 0, None, None) != 0
    assert b"N < 0" in lib.texgs_last_error()
    assert lib.texgs_cube_sample(None, 4, 3, None, 4, 2, 0, None, None) != 0
    assert b"filter" in lib.texgs_last_error()
    assert lib.texgs_cube_sample(None, 4, 3, None, 4, 0, 0, None, None) != 0
    assert b"NULL" in lib.texgs_last_error()
    assert lib.texgs_cube_latlong(None, 4, 3, 0, 8, 0, None, None) != 0
    assert b"H and W" in lib.texgs_last_error()
    assert lib.texgs_cube_latlong(None, 4, 3, 2 ** 16, 2 ** 15, 0, None, None) != 0
    assert b"H W" in lib.texgs_last_error()
    assert lib.texgs_cube_latlong(None, 4, 3, 4, 8, 0, None, None) != 0
    assert b"NULL" in lib.texgs_last_error()
    assert lib.texgs_cube_sample_backward(None, 4, 3, None, 4, None, None, None, None) != 0
    assert b"both NULL" in lib.texgs_last_error()
    assert lib.texgs_cube_sample_backward(None, 1, 3, None, 4, None, None, None, None) != 0
    assert b"R < 2" in lib.texgs_last_error()


def test_library_exports_the_entry_points(lib_built):
    lib = ctypes.CDLL(lib_built)
    from texgs import _lib
    for name in ENTRY_POINTS + ("texgs_cube_sample_nearest_backward",):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def test_stale_library_is_told_to_rebuild(tmp_path):
    """A libtexgs.so from before these additions (same ABI version, fewer symbols) raises the loader's "rebuild it" RuntimeError,
    not an AttributeError from ctypes."""
    src = tmp_path / "stale.c"
    src.write_text("int texgs_abi_version(void) { return 18; }\nconst char* texgs_last_error(void) { return \"\"; }\n")
    so = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    code = ("import sys; sys.path[:0]=[%r]\nfrom texgs import _lib\n"
            "try:\n    _lib.load()\nexcept RuntimeError as e:\n    assert 'texgs_cube_sample' in str(e) and 'rebuild it' in str(e), e\n"
            "else:\n    raise SystemExit('loaded a stale library')" % os.path.join(ROOT, "texture-gs_amd"))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, TEXGS_LIB=str(so)))


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "texgs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(\s*const float\*\s*tex,\s*int32_t R,\s*int32_t C," % name, hdr), name
    assert re.search(r"#define\s+TEXGS_ABI_VERSION\s+19\b", hdr)


def test_nvdiffrast_drop_in_refuses_what_it_does_not_do():
    sys.path.insert(0, os.path.join(ROOT, "texture-gs_amd"))
    import nvdiffrast.torch as dr
    tex = torch.rand(1, 6, 4, 4, 3)
    uv = torch.rand(1, 2, 5, 3)
    with pytest.raises(NotImplementedError, match="boundary_mode='wrap'"):
        dr.texture(tex, uv, boundary_mode="wrap")
    with pytest.raises(NotImplementedError, match="boundary_mode='wrap'"):
        dr.texture(tex, uv)                                           # the package's default
    with pytest.raises(NotImplementedError, match="mip is not supported"):
        dr.texture(tex, uv, mip=[tex], boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="uv_da is not supported"):
        dr.texture(tex, uv, uv_da=torch.rand(1, 2, 5, 6), boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="mip_level_bias is not supported"):
        dr.texture(tex, uv, mip_level_bias=torch.rand(1, 2, 5), boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="max_mip_level is not supported"):
        dr.texture(tex, uv, max_mip_level=2, boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="filter_mode='linear-mipmap-linear'"):
        dr.texture(tex, uv, filter_mode="linear-mipmap-linear", boundary_mode="cube")
    with pytest.raises(NotImplementedError, match="2-D textures"):
        dr.texture(tex[:, 0], uv, boundary_mode="cube")
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # a supported call reaches texgs.cubetex, which has no CPU path
        dr.texture(tex, uv, boundary_mode="cube")
