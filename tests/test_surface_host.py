"""-m "not gpu": the surface-point stage (texgs/surface.py, include/texgs_surface.h) without a GPU.

* The numpy statement (tests/surface_ref.py) against the reference's own float64 points (tests/golden/host_terms.npz), against
  numpy's inverse, and its compaction and composite against independent numpy on hand-made masks.
* Structure: the ctypes mirrors against gcc's layout of the header's structs, the header as plain C99, the exports and their
  signatures against the prototypes, the C entries' refusals (they need no GPU), the build script's knowledge of the unit.
* Every validation error of texgs.surface is raised on CPU tensors BEFORE the "no CPU fallback" error."""
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
import surface_ref as R  # noqa: E402
from texgs import surface as _surface  # noqa: E402,F401  (the feature under test: without it this file fails at import)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_surface.h")
HT = os.path.join(ROOT, "tests", "golden", "host_terms.npz")


# ---- the statement ----
def test_statement_lands_on_the_reference_float64_points():
    """All pixels selected: within 1e-6 + 2^-24 |x| of d2w_xyz64 -- the bound tests/test_losses.py holds the fp64 formula to, plus the
    one rounding to float32.  (Measured where this was written: 1.6e-7; an fp32 product with the same inverse: 6.2e-5.)"""
    d = np.load(HT)
    depth, proj, zfar, znear = d["d2w_depth"], d["d2w_full_proj"], float(d["d2w_zfar"]), float(d["d2w_znear"])
    assert depth.shape == (17, 23) and proj.dtype == np.float32
    got = R.surface_points(depth, np.ones((17, 23), R.F), proj, zfar, znear)
    assert got["count"] == 17 * 23 and got["xyz"].dtype == np.float32
    want = d["d2w_xyz64"].reshape(-1, 3)
    err = np.abs(got["xyz"].astype(np.float64) - want)
    print("largest difference from d2w_xyz64:", err.max())
    assert (err <= 1e-6 + 2.0 ** -24 * np.abs(want)).all(), err.max()
    # the fp32 path this stage replaces is two orders of magnitude further away
    assert np.abs(d["d2w_xyz"].reshape(-1, 3).astype(np.float64) - want).max() > 50 * err.max()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_inverse_columns_invert(seed):
    d = np.load(HT)
    for proj in (d["d2w_full_proj"], R.camera(17, 23, seed)[0]):
        B = R.inverse_columns(proj)
        assert B.shape == (4, 3) and B.dtype == np.float64
        want = np.linalg.inv(proj.astype(np.float64))[:, :3]
        assert np.abs(B - want).max() <= 1e-9 * np.abs(want).max()
    # a singular matrix: non-finite, not an error
    assert not np.isfinite(R.inverse_columns(np.zeros(16, R.F))).any()


def hand_masks():
    a = np.full((5, 7), 0.25, R.F)
    out = {"none": a.copy(), "all": np.full((5, 7), 0.75, R.F)}
    m = a.copy(); m[0, 0] = 1; out["first"] = m
    m = a.copy(); m[4, 6] = 1; out["last"] = m
    m = a.copy(); m.reshape(-1)[::2] = 0.9; out["alternate"] = m
    m = a.copy(); m[1, 2:5] = 0.6; m[3, 0] = np.inf; m[3, 1] = np.nan; m[3, 2] = 0.5; m[3, 3] = np.nextafter(R.F(0.5), R.F(1)); m[3, 4] = -0.0
    out["hand"] = m
    return out


@pytest.mark.parametrize("name", list(hand_masks()))
def test_compaction_and_composite_on_hand_made_masks(name):
    alpha = hand_masks()[name]
    H, W = alpha.shape
    depth = R.make_depth(H, W, seed=3)
    proj, zfar, znear = R.camera(H, W, seed=3)
    got = R.surface_points(depth, alpha, proj, zfar, znear)
    with np.errstate(invalid="ignore"):
        want_index = np.flatnonzero(alpha.reshape(-1) > 0.5)
    assert np.array_equal(got["index"], want_index) and got["index"].dtype == np.int64 and got["count"] == want_index.size
    if name == "hand":
        assert want_index.tolist() == [9, 10, 11, 21, 24]           # inf and nextafter(0.5) in; NaN, 0.5 and -0 out
    # rank is the inverse of index
    rank = got["rank"]
    assert rank.dtype == np.int32 and rank.shape == (H * W,)
    assert np.array_equal(rank[got["index"]], np.arange(got["count"]))
    assert (np.delete(rank, got["index"]) == -1).all()
    assert np.array_equal(got["alpha"], alpha.reshape(-1)[want_index])
    assert np.array_equal(got["xyz"], R.world_points(depth, proj, zfar, znear)[want_index])
    # the composite against a scatter built independently
    rng = np.random.default_rng(5)
    values = rng.random((got["count"], 3)).astype(R.F)
    for bg in (None, R.BACKGROUND):
        out = R.compose(values, rank, alpha, bg)
        assert out.shape == (3, H, W) and out.dtype == np.float32
        b = np.zeros(3, R.F) if bg is None else bg
        a = alpha.reshape(-1)
        with np.errstate(invalid="ignore"):
            want = (b[None, :] * (R.F(1) - a)[:, None]).astype(R.F)                 # [HW,3] background term
            scattered = np.zeros((H * W, 3), R.F)
            for r, p in enumerate(want_index):
                scattered[p] = a[p] * values[r]
            want = (want + scattered).T.reshape(3, H, W)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    if got["count"] == 0:
        assert np.array_equal(R.compose(values, rank, alpha, R.BACKGROUND),
                              (R.BACKGROUND[:, None, None] * (R.F(1) - alpha)[None]).astype(R.F) + R.F(0))


def test_ndc_and_depth_terms_follow_the_reference_formula():
    """The statement's points project back onto the pixel grid at view depth d (the inverse really is the projection's)"""
    H, W = 9, 13
    depth = R.make_depth(H, W, seed=1)
    proj, zfar, znear = R.camera(H, W, seed=1)
    xyz = R.world_points(depth, proj, zfar, znear).astype(np.float64)
    clip = np.concatenate([xyz, np.ones((H * W, 1))], axis=1) @ proj.astype(np.float64)
    gx = np.tile((np.arange(W) * 2 + 1) / W - 1, H)
    gy = np.repeat((np.arange(H) * 2 + 1) / H - 1, W)
    # 1e-4 as in tests/test_losses.py: the float32 matrix's z column is the formula's zfar / (zfar - znear) only to float32, and the
    # inverse amplifies that by the near-parallel z and w columns
    assert np.abs(clip[:, 0] / clip[:, 3] - gx).max() < 1e-4 and np.abs(clip[:, 1] / clip[:, 3] - gy).max() < 1e-4
    assert np.abs(clip[:, 3] - depth.reshape(-1)).max() < 1e-4


# ---- structure ----
def test_structs_match_c_layout(tmp_path):
    from texgs import surface
    consts = {"TEXGS_SURFACE_PIXELS_PER_THREAD": surface.PIXELS_PER_THREAD, "TEXGS_SURFACE_PIXELS_PER_WORKGROUP": surface.PIXELS_PER_WORKGROUP,
              "TEXGS_SURFACE_SCAN_WIDTH": surface.SCAN_WIDTH, "TEXGS_SURFACE_MAX_SIDE": surface.MAX_SIDE}
    assert sorted(surface.MIRRORS) == ["TexGSSurfaceCompose", "TexGSSurfacePoints"]
    assert abi_check.layout_mismatches("texgs_surface.h", surface.MIRRORS, consts, tmp_path) == []


def test_header_is_plain_c99_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_surface.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert "TEXGS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "texgs_surface.h"' in open(os.path.join(ROOT, "texture-gs_amd", "csrc", "surface.hip")).read()
    assert re.search(r"#define TEXGS_ABI_VERSION 19\b", open(os.path.join(INC, "texgs.h")).read())


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib, surface
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(surface.SIGNATURES) == sorted(["texgs_surface_temp_bytes", "texgs_surface_points", "texgs_surface_compose"])
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, surface.SIGNATURES, surface.MIRRORS) == []
    lib = surface.entry()
    assert lib is _lib.load() and lib.texgs_surface_points.argtypes == surface.SIGNATURES["texgs_surface_points"][1]
    assert lib.texgs_abi_version() == 19
    # the mirrors and the signatures live in texgs/surface.py, not in the table that tests/test_abi.py pins to texgs.h
    assert not any(n in _lib.SIGNATURES for n in protos) and not hasattr(_lib, "SurfacePointsStruct")
    # the build knows the unit: its flag, the header as a dependency of every unit and as part of the build id
    build = abi_check.build_knows_header(HDR)
    assert build.UNITS["surface.hip"] == ["-ffp-contract=off"]


def test_c_entries_refuse_bad_arguments_before_any_launch(lib_built):
    """No GPU here: a call that got as far as a launch would fail with a HIP error instead of the cause named below."""
    from texgs import surface
    lib = surface.entry()
    buf = (C.c_double * 64)()            # stands in for every device buffer: nothing may read it
    b = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.texgs_last_error().decode()
    B, S = surface.PIXELS_PER_WORKGROUP, surface.SCAN_WIDTH
    tb = lib.texgs_surface_temp_bytes
    assert tb(0, 5) == 0 and tb(5, -1) == 0 and tb(16385, 1) == 0 and tb(1, 16385) == 0
    assert tb(1, 1) == 256 and tb(1, B) == 256 and tb(40, B) == 256 and tb(41, B) == 512        # 96 bytes of inverse, then a word per workgroup
    assert tb(16384, 16384) == (96 + 4 * (16384 * 16384 // B) + 255) // 256 * 256
    P = lambda **kw: surface.SurfacePointsStruct(**{**dict(depth=b, alpha=b, full_proj=b, xyz=b, index=b, alpha_sel=b, rank=b, count=b,
                                                           zfar=100.0, znear=0.01, threshold=0.5, height=2, width=3, capacity=6), **kw})
    for kw, temp, nbytes, cause in [
            (dict(depth=None), b, 256, "NULL argument"), (dict(alpha=None), b, 256, "NULL argument"), (dict(full_proj=None), b, 256, "NULL argument"),
            (dict(xyz=None), b, 256, "NULL argument"), (dict(count=None), b, 256, "NULL argument"), (dict(), None, 256, "NULL argument"),
            (dict(height=0), b, 256, "must be positive"), (dict(width=-3), b, 256, "must be positive"),
            (dict(height=16385, capacity=2 ** 31 - 1), b, 1 << 20, "above 16384"), (dict(width=16385, capacity=2 ** 31 - 1), b, 1 << 20, "above 16384"),
            (dict(zfar=3.0, znear=3.0), b, 256, "two different numbers"), (dict(zfar=float("nan")), b, 256, "two different numbers"),
            (dict(threshold=float("nan")), b, 256, "threshold is NaN"),
            (dict(capacity=5), b, 256, "capacity must be at least"), (dict(capacity=-1), b, 256, "capacity must be at least"),
            (dict(), b, 255, "temp is smaller"), (dict(height=41, width=B, capacity=41 * B), b, 256, "temp is smaller"),
            (dict(depth=b + 2), b, 256, "4-byte aligned"), (dict(rank=b + 1), b, 256, "4-byte aligned"),
            (dict(index=b + 4), b, 256, "8-byte aligned"), (dict(), b + 4, 256, "8-byte aligned")]:
        assert lib.texgs_surface_points(C.byref(P(**kw)), temp, nbytes, None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_surface_points(None, b, 256, None) != 0 and "NULL" in err()
    X = lambda **kw: surface.SurfaceComposeStruct(**{**dict(values=b, rank=b, alpha=b, background=None, out=b, rows=3, height=2, width=3), **kw})
    for kw, cause in [(dict(values=None), "NULL argument"), (dict(rank=None), "NULL argument"), (dict(alpha=None), "NULL argument"),
                      (dict(out=None), "NULL argument"), (dict(rows=-1), "rows < 0"), (dict(height=0), "must be positive"),
                      (dict(width=16385), "above 16384"), (dict(background=b + 2), "4-byte aligned"), (dict(out=b + 1), "4-byte aligned")]:
        assert lib.texgs_surface_compose(C.byref(X(**kw)), None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_surface_compose(None, None) != 0 and "NULL" in err()
    assert S * B == 262144          # the shapes of tests/test_surface_gpu.py are sized from these


# ---- texgs.surface refuses by name, before the "no CPU fallback" error ----
def _cpu_points(H, W, M, rank=True):
    from texgs import surface as Sm
    pts = Sm.SurfacePoints(H, W, torch.zeros(H * W, 3), None, None, torch.full((H, W), -1, dtype=torch.int32) if rank else None, None, None)
    pts._count = M
    return pts


def test_every_validation_error_comes_before_the_cpu_refusal():
    from texgs import surface as Sm
    d, a, P = torch.ones(4, 5), torch.ones(4, 5), torch.eye(4)
    sp = lambda depth=d, alpha=a, proj=P, zfar=100.0, znear=0.01, **kw: Sm.surface_points(depth, alpha, proj, zfar, znear, **kw)
    pts = _cpu_points(4, 5, 2)
    vals = torch.zeros(2, 3)
    bad = [
        (TypeError, "depth must be a torch.Tensor", lambda: sp(depth=np.ones((4, 5), np.float32))),
        (ValueError, r"depth must be \[H,W\] or \[1,H,W\]", lambda: sp(depth=torch.ones(2, 4, 5))),
        (ValueError, r"depth must be \[H,W\] or \[1,H,W\]", lambda: sp(depth=torch.ones(20))),
        (ValueError, "depth must be torch.float32", lambda: sp(depth=d.double())),
        (ValueError, "depth must be contiguous", lambda: sp(depth=torch.ones(5, 4).t())),
        (ValueError, r"each side must be in \[1,16384\]", lambda: sp(depth=torch.ones(0, 5), alpha=torch.ones(0, 5))),
        (ValueError, r"each side must be in \[1,16384\]", lambda: sp(depth=torch.ones(1, 16385), alpha=torch.ones(1, 16385))),
        (TypeError, "alpha must be a torch.Tensor", lambda: sp(alpha=None)),
        (ValueError, r"alpha must be \[4,5\] or \[1,4,5\]", lambda: sp(alpha=torch.ones(5, 4))),
        (ValueError, "alpha must be torch.float32", lambda: sp(alpha=a > 0)),
        (ValueError, "alpha must be contiguous", lambda: sp(alpha=torch.ones(4, 10)[:, ::2])),
        (TypeError, "full_proj_transform must be a torch.Tensor", lambda: sp(proj=np.eye(4, dtype=np.float32))),
        (ValueError, r"full_proj_transform must be \[4,4\]", lambda: sp(proj=torch.ones(16))),
        (ValueError, "full_proj_transform must be torch.float32", lambda: sp(proj=P.double())),
        (ValueError, "full_proj_transform must be contiguous", lambda: sp(proj=torch.ones(4, 4).t())),
        (TypeError, "zfar must be a number", lambda: sp(zfar="100")),
        (TypeError, "znear must be a number", lambda: sp(znear=torch.tensor(0.01))),
        (ValueError, "two different numbers", lambda: sp(zfar=1.0, znear=1.0)),
        (ValueError, "two different numbers", lambda: sp(zfar=float("nan"))),
        (TypeError, "threshold must be a number", lambda: sp(threshold=None)),
        (ValueError, "threshold is NaN", lambda: sp(threshold=float("nan"))),
        (TypeError, "points must be a SurfacePoints", lambda: Sm.compose(torch.zeros(4, 5), vals, a)),
        (ValueError, "with_rank=True", lambda: Sm.compose(_cpu_points(4, 5, 2, rank=False), vals, a)),
        (ValueError, r"alpha must be \[4,5\] or \[1,4,5\]", lambda: Sm.compose(pts, vals, torch.ones(5, 5))),
        (TypeError, "values must be a torch.Tensor", lambda: Sm.compose(pts, [[0, 0, 0]] * 2, a)),
        (ValueError, r"values must be \[M,3\]", lambda: Sm.compose(pts, torch.zeros(2, 4), a)),
        (ValueError, "values must be torch.float32", lambda: Sm.compose(pts, vals.half(), a)),
        (ValueError, "values must be contiguous", lambda: Sm.compose(pts, torch.zeros(3, 2).t(), a)),
        (ValueError, "background must hold 3 values", lambda: Sm.compose(pts, vals, a, background=[0, 1])),
        (ValueError, "background must hold 3 values", lambda: Sm.compose(pts, vals, a, background=torch.zeros(4))),
        (TypeError, "background must be a tensor or a sequence", lambda: Sm.compose(pts, vals, a, background=0.5)),
    ]
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()
    # valid arguments on the CPU: refused as such, never computed in torch
    for call in (lambda: sp(), lambda: sp(depth=d[None], alpha=a[None], threshold=0.25, with_alpha=True, with_rank=True, wait=False),
                 lambda: Sm.compose(pts, vals, a), lambda: Sm.compose(pts, vals, a[None], background=[0, 0.5, 1]),
                 lambda: Sm.chess_image(d, a, P, 100.0, 0.01, None, torch.zeros(128))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_uv_map_loss_checks_world_xyz_before_anything_runs():
    from texgs import uvmap
    d, a = torch.ones(1, 4, 5), torch.ones(1, 4, 5)
    for exc, pattern, w in [(TypeError, "world_xyz must be a torch.Tensor", np.zeros((3, 3), np.float32)),
                            (ValueError, r"world_xyz must be float32 \[M, 3\]", torch.zeros(3, 4)),
                            (ValueError, r"world_xyz must be float32 \[M, 3\]", torch.zeros(3, 3, dtype=torch.float64))]:
        with pytest.raises(exc, match=pattern):
            uvmap.uv_map_loss(d, a, torch.eye(4), 0.01, 100.0, None, None, torch.zeros(128), None, world_xyz=w)
