"""-m "not gpu": the output stage (texgs/present.py, include/texgs_present.h) without a GPU.

* The numpy statement (tests/present_ref.py) equals the reference's own lines in torch-CPU float32 on the inputs the GPU tests use:
  bytes bit for bit, floats as values (torch.clamp may return either zero for -0; the statement keeps -0).
* Structure: the ctypes mirrors against gcc's layout of the header's structs, the header as plain C99, the exports and their
  signatures against the prototypes, the C entries' refusals (they need no GPU), the build script's knowledge of the unit.
* Every validation error of texgs.present is raised on CPU tensors BEFORE the "no CPU fallback" error; jet_lut's values and its
  one warning; FrameReader's argument checks."""
import ctypes as C
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import present_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_present.h")
SHAPES = [(1, 1), (7, 9), (33, 65), (64, 64)]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- the statement is the reference ----
@pytest.mark.parametrize("H,W", SHAPES)
def test_statement_is_retexture(H, W):
    img, alpha = R.make_image(3, H, W, seed=1), R.make_alpha(H, W)
    want = R.reference_retexture(t(img), t(alpha)[None], t(R.BACKGROUND))
    assert np.array_equal(R.frame_u8(img, alpha, R.BACKGROUND), want)
    # no mask: the reference composites with ones, the statement does not composite at all -- the same bytes
    assert np.array_equal(R.frame_u8(img), R.reference_retexture(t(img), None, t(R.BACKGROUND)))
    assert np.array_equal(R.frame_u8(img, np.ones((H, W), R.F), R.BACKGROUND), R.frame_u8(img))
    # cv2.cvtColor(RGB2BGR) is the channel swap
    assert np.array_equal(R.frame_u8(img, alpha, R.BACKGROUND, order="bgr"), want[:, :, ::-1])
    four = R.frame_u8(img, alpha, R.BACKGROUND, channels=4)
    assert np.array_equal(four[:, :, :3], want) and (four[:, :, 3] == 255).all()


def test_quantise_truncates_and_saturates():
    v = np.array([0, -0.0, 1, 1 - 2.0 ** -24, 256 / 255, 0.5, -3, 7, np.nan, np.inf, -np.inf, 254.99 / 255], dtype=R.F)
    assert R.quantise(v).tolist() == [0, 0, 255, 254, 255, 127, 0, 255, 0, 255, 0, 254]
    pv = R.planted_values()
    assert np.array_equal(R.quantise(pv), np.minimum(np.trunc(pv.astype(np.float32) * np.float32(255)), 255).astype(np.uint8))
    c = R.clamp01(np.array([-0.0, np.nan, 2, -1], dtype=R.F))
    assert np.signbit(c[0]) and np.isnan(c[1]) and c[2] == 1 and c[3] == 0 and not np.signbit(c[3])


@pytest.mark.parametrize("H,W", SHAPES)
def test_statement_is_the_depth_picture(H, W):
    lut = R.random_lut()
    depth = R.make_depth(H, W, seed=2)
    masks = {"none": None, "ones": np.ones((H, W), R.F), "fraction": np.where(R.make_alpha(H, W) > 0, R.F(0.25), R.F(0))}
    single = np.zeros((H, W), R.F)
    single[H // 2, W // 2] = 1
    masks["single"] = single
    if H * W == 1:
        masks.pop("fraction")                   # (its only pixel is off: the reference raises on an empty selection)
    for name, m in masks.items():
        rgb, (lo, hi) = R.depth_colour(depth, m, lut)
        want = R.reference_depth(t(depth)[None], None if m is None else t(m)[None], lut).numpy()
        assert np.array_equal(R.bytes_as_float(rgb), want), name
        sel = depth[m != 0] if m is not None else depth
        assert lo == sel.min() and hi == sel.max()
    rgb, rng = R.depth_colour(depth, np.zeros((H, W), R.F), lut)
    assert not rgb.any() and rng == (np.inf, -np.inf)


def test_statement_depth_near_ties_and_flat():
    lut = R.random_lut()
    d = R.near_tie_depth()
    rgb, (lo, hi) = R.depth_colour(d, None, lut)
    assert (lo, hi) == (0, 255)
    assert np.array_equal(R.bytes_as_float(rgb), R.reference_depth(t(d)[None], None, lut).numpy())
    flat = np.full((5, 7), 3.25, R.F)
    rgb, _ = R.depth_colour(flat, None, lut)
    assert np.array_equal(R.bytes_as_float(rgb), R.reference_depth(t(flat)[None], None, lut).numpy())
    assert (rgb == lut[0][:, None, None]).all()


@pytest.mark.parametrize("H,W", SHAPES)
def test_statement_is_the_viewer_frame(H, W):
    lut = R.random_lut()
    img, norm = R.make_image(3, H, W, seed=3), R.make_image(3, H, W, seed=4, affine=True)
    alpha, depth = R.make_image(1, H, W, seed=5), R.make_depth(H, W, seed=6)
    mask = np.where(alpha[0] > 0.3, alpha[0], R.F(0)) if H * W > 1 else np.ones((1, 1), R.F)
    pkg = dict(image=t(img), norm=t(norm), alpha=t(alpha), depth=t(depth)[None])
    assert np.array_equal(R.hwc4(R.present_values(img)), R.reference_viewer(pkg, "rgb").numpy())
    assert np.array_equal(R.hwc4(R.present_values(norm, affine=True)), R.reference_viewer(pkg, "norm").numpy())
    assert np.array_equal(R.hwc4(R.present_values(alpha)), R.reference_viewer(pkg, "alpha").numpy())
    pkg["alpha"] = t(mask)[None]
    got = R.hwc4(R.bytes_as_float(R.depth_colour(depth, mask, lut)[0]))
    assert np.array_equal(got, R.reference_viewer(pkg, "depth", lut).numpy())


@pytest.mark.parametrize("res", [1, 3, 16])
def test_statement_is_the_cross(res):
    tex = R.make_texture(res, seed=7)
    got = R.cross_u8(tex)
    assert got.shape == (3 * res, 4 * res, 3) and np.array_equal(got, R.reference_cross(t(tex)))
    assert not got[:res, :res].any() and not got[2 * res:, 2 * res:].any()


# ---- structure ----
def test_structs_match_c_layout(tmp_path):
    from texgs import present
    consts = {"TEXGS_PRESENT_PIXELS_PER_THREAD": present.PIXELS_PER_THREAD, "TEXGS_PRESENT_PIXELS_PER_WORKGROUP": present.PIXELS_PER_WORKGROUP,
              "TEXGS_PRESENT_MAX_WORKGROUPS": present.MAX_WORKGROUPS, "TEXGS_PRESENT_AFFINE": present.AFFINE,
              "TEXGS_PRESENT_COMPOSITE": present.COMPOSITE, "TEXGS_PRESENT_SWAP_RB": present.SWAP_RB}
    assert sorted(present.MIRRORS) == ["TexGSCubeCross", "TexGSDepthColour", "TexGSPresent"]
    assert abi_check.layout_mismatches("texgs_present.h", present.MIRRORS, consts, tmp_path) == []


def test_header_is_plain_c99_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_present.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert "TEXGS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "texgs_present.h"' in open(os.path.join(ROOT, "texture-gs_amd", "csrc", "present.hip")).read()


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib, present
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(present.SIGNATURES) == sorted(["texgs_present", "texgs_depth_colour_temp_bytes", "texgs_depth_colour",
                                                                    "texgs_cube_cross"])
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, present.SIGNATURES, present.MIRRORS) == []
    lib = present.entry()
    assert lib is _lib.load() and lib.texgs_present.argtypes == present.SIGNATURES["texgs_present"][1]
    # the mirrors and the signatures live in texgs/present.py, not in the table that tests/test_abi.py pins to texgs.h
    assert not any(n in _lib.SIGNATURES for n in protos) and not hasattr(_lib, "PresentStruct")
    # the build knows the unit: its flag, the header as a dependency of every unit and as part of the build id
    build = abi_check.build_knows_header(HDR)
    assert build.UNITS["present.hip"] == ["-ffp-contract=off"]


def test_c_entries_refuse_bad_arguments_before_any_launch(lib_built):
    """No GPU here: a call that got as far as a launch would fail with a HIP error instead of the cause named below."""
    from texgs import present
    lib = present.entry()
    buf = (C.c_float * 64)()            # stands in for every device buffer: nothing may read it
    b = C.addressof(buf)
    b = (b + 15) & ~15
    err = lambda: lib.texgs_last_error().decode()
    P = lambda **kw: present.PresentStruct(**{**dict(src=b, alpha=b, background=b, out_u8=b, out_hwc4=None, out_chw=None, height=2, width=2,
                                                     channels=3, u8_channels=3, flags=0), **kw})
    for kw, cause in [(dict(src=None), "NULL argument (src)"), (dict(channels=2), "channels must be 1 or 3"),
                      (dict(u8_channels=5), "u8_channels must be 3 or 4"), (dict(out_u8=None), "no output requested"),
                      (dict(flags=present.COMPOSITE, alpha=None), "composite mode needs alpha"), (dict(height=0), "must be positive"),
                      (dict(width=-1), "must be positive"), (dict(height=65536, width=32768), "below 2^31"),
                      (dict(flags=8), "unknown bit"), (dict(out_u8=b + 2), "out_u8 must be"), (dict(out_u8=b + 4, u8_channels=4), "out_u8 must be"),
                      (dict(out_hwc4=b + 4), "out_hwc4 must be 16-byte aligned"), (dict(out_chw=b + 1), "out_chw must be 4-byte aligned"),
                      (dict(src=b + 1), "4-byte aligned")]:
        assert lib.texgs_present(C.byref(P(**kw)), None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_present(None, None) != 0 and "NULL" in err()
    assert lib.texgs_depth_colour_temp_bytes(0, 5) == 0 and lib.texgs_depth_colour_temp_bytes(65536, 32768) == 0
    assert lib.texgs_depth_colour_temp_bytes(1, 1) == 8 and lib.texgs_depth_colour_temp_bytes(32, 33) == 16
    assert lib.texgs_depth_colour_temp_bytes(4096, 4096) == 8 * present.MAX_WORKGROUPS
    D = lambda **kw: present.DepthColourStruct(**{**dict(depth=b, mask=None, lut=b, range=b, out_u8=None, out_hwc4=None, out_chw=b, height=2,
                                                         width=2, u8_channels=3, flags=0), **kw})
    for kw, temp, nbytes, cause in [(dict(depth=None), b, 8, "NULL argument"), (dict(lut=None), b, 8, "NULL argument"), (dict(), None, 8, "NULL argument"),
                                    (dict(out_chw=None), b, 8, "no output requested"), (dict(), b, 7, "temp is smaller"),
                                    (dict(height=40, width=40), b, 8, "temp is smaller"), (dict(flags=present.AFFINE), b, 8, "unknown bit"),
                                    (dict(out_u8=b, u8_channels=0), b, 8, "u8_channels"), (dict(height=0), b, 8, "must be positive"),
                                    (dict(range=b + 2), b, 8, "4-byte aligned")]:
        assert lib.texgs_depth_colour(C.byref(D(**kw)), temp, nbytes, None) != 0, kw
        assert cause in err(), (kw, err())
    X = lambda **kw: present.CubeCrossStruct(**{**dict(texture=b, out=b, res=4), **kw})
    for kw, cause in [(dict(res=0), "res must be"), (dict(res=7169), "res must be"), (dict(texture=None), "NULL argument"),
                      (dict(out=None), "NULL argument"), (dict(out=b + 1), "4-byte aligned")]:
        assert lib.texgs_cube_cross(C.byref(X(**kw)), None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_cube_cross(None, None) != 0 and lib.texgs_depth_colour(None, b, 8, None) != 0


# ---- texgs.present refuses by name, before the "no CPU fallback" error ----
def test_every_validation_error_comes_before_the_cpu_refusal():
    from texgs import present as Pm
    img, plane = torch.zeros(3, 4, 5), torch.zeros(4, 5)
    lut = torch.zeros(256, 3, dtype=torch.uint8)
    bad = [
        (TypeError, "image must be a torch.Tensor", lambda: Pm.frame_u8(np.zeros((3, 4, 5), np.float32))),
        (ValueError, r"image must be \[C,H,W\]", lambda: Pm.frame_u8(torch.zeros(2, 4, 5))),
        (ValueError, r"image must be \[C,H,W\]", lambda: Pm.frame_u8(torch.zeros(4, 5))),
        (ValueError, "image must be torch.float32", lambda: Pm.frame_u8(img.double())),
        (ValueError, "image must be contiguous", lambda: Pm.frame_u8(torch.zeros(3, 5, 4).transpose(1, 2))),
        (ValueError, r"H\*W must be in", lambda: Pm.frame_u8(torch.zeros(3, 0, 5))),
        (ValueError, r"alpha must be \[4,5\] or \[1,4,5\]", lambda: Pm.frame_u8(img, alpha=torch.zeros(5, 4))),
        (ValueError, "alpha must be torch.float32", lambda: Pm.frame_u8(img, alpha=plane.half())),
        (TypeError, "alpha must be a torch.Tensor", lambda: Pm.frame_u8(img, alpha=1.0)),
        (ValueError, "background must hold 3 values", lambda: Pm.frame_u8(img, alpha=plane, background=[0, 1])),
        (ValueError, "background must hold 3 values", lambda: Pm.frame_u8(img, alpha=plane, background=torch.zeros(4))),
        (TypeError, "background must be a tensor or a sequence", lambda: Pm.frame_u8(img, alpha=plane, background=0.5)),
        (ValueError, "order must be", lambda: Pm.frame_u8(img, order="gbr")),
        (ValueError, "channels must be 3 or 4", lambda: Pm.frame_u8(img, channels=1)),
        (TypeError, "channels must be an int", lambda: Pm.frame_u8(img, channels=3.0)),
        (ValueError, "out must be a contiguous torch.uint8", lambda: Pm.frame_u8(img, out=torch.zeros(4, 5, 4, dtype=torch.uint8))),
        (ValueError, "out must be a contiguous torch.uint8", lambda: Pm.frame_u8(img, out=torch.zeros(4, 5, 3))),
        (ValueError, "mode must be one of", lambda: Pm.display(img, mode="uv")),
        (TypeError, "x must be a torch.Tensor", lambda: Pm.display(None)),
        (ValueError, r"x must be \[C,H,W\] with C in \(3,\)", lambda: Pm.display(plane[None], mode="norm")),
        (ValueError, r"x must be \[C,H,W\] with C in \(1,\)", lambda: Pm.display(img, mode="alpha")),
        (ValueError, "out must be a contiguous torch.float32", lambda: Pm.display(img, out=torch.zeros(4, 5, 3))),
        (ValueError, "lut must be a contiguous uint8", lambda: Pm.display(plane, mode="depth", lut=torch.zeros(256, 3))),
        (ValueError, "alpha must be", lambda: Pm.display(plane, mode="depth", alpha=torch.zeros(2, 2))),
        (TypeError, "depth must be a torch.Tensor", lambda: Pm.depth_colour([1.0])),
        (ValueError, r"depth must be \[C,H,W\]", lambda: Pm.depth_colour(img)),
        (ValueError, "mask must be", lambda: Pm.depth_colour(plane, mask=torch.zeros(3, 4, 5))),
        (ValueError, r"lut must be uint8 \[256,3\]", lambda: Pm.depth_colour(plane, lut=np.zeros((256, 3), np.float32))),
        (ValueError, "lut must be a contiguous uint8", lambda: Pm.depth_colour(plane, lut=torch.zeros(255, 3, dtype=torch.uint8))),
        (TypeError, "lut must be a torch.Tensor or a numpy array", lambda: Pm.depth_colour(plane, lut="jet")),
        (TypeError, "x must be a torch.Tensor", lambda: Pm.to_chw01(3)),
        (ValueError, "x must be torch.float32", lambda: Pm.to_chw01(img.int())),
        (TypeError, "texture must be a torch.Tensor", lambda: Pm.cross_u8(None)),
        (ValueError, r"texture must be \[6,R,R,3\]", lambda: Pm.cross_u8(torch.zeros(6, 4, 5, 3))),
        (ValueError, r"texture must be \[6,R,R,3\]", lambda: Pm.cross_u8(torch.zeros(5, 4, 4, 3))),
        (ValueError, "texture must be torch.float32", lambda: Pm.cross_u8(torch.zeros(6, 4, 4, 3, dtype=torch.float64))),
        (ValueError, "out must be a contiguous torch.uint8", lambda: Pm.cross_u8(torch.zeros(6, 4, 4, 3), out=torch.zeros(12, 16, 4, dtype=torch.uint8))),
    ]
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()
    # valid arguments on the CPU: refused as such, never computed in torch
    tex = torch.zeros(6, 4, 4, 3)
    for call in (lambda: Pm.frame_u8(img), lambda: Pm.frame_u8(img, alpha=plane > 0, background=[0, 0.5, 1], order="bgr", channels=4),
                 lambda: Pm.display(img), lambda: Pm.display(plane, mode="alpha"), lambda: Pm.display(plane, mode="depth", alpha=plane, lut=lut),
                 lambda: Pm.depth_colour(plane, mask=plane, lut=lut), lambda: Pm.depth_colour(plane[None], lut=np.zeros((256, 3), np.uint8)),
                 lambda: Pm.to_chw01(img, affine=True), lambda: Pm.to_chw01(plane), lambda: Pm.cross_u8(tex)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_jet_lut_values_and_its_single_warning():
    from texgs import present as Pm
    table = Pm.jet_table()
    assert table.shape == (256, 3) and table.dtype == np.uint8
    want = {0: (0, 0, 128), 32: (0, 1, 255), 96: (2, 255, 254), 128: (130, 255, 126), 160: (255, 253, 0), 224: (252, 0, 0), 255: (128, 0, 0)}
    assert {i: tuple(int(v) for v in table[i]) for i in want} == want
    # the definition in floating point: clip(1.5 - |4x - c|, 0, 1) * 255, rounded half up
    x = np.arange(256) / 255.0
    for k, c in enumerate((3, 2, 1)):
        f = np.clip(1.5 - np.abs(4 * x - c), 0, 1) * 255
        assert np.abs(table[:, k] - f).max() <= 0.5 + 1e-9
    Pm._jet_warned = False
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a, b = Pm.jet_lut("cpu"), Pm.jet_lut("cpu")
    texts = [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(texts) == 1 and "UNPINNED" in texts[0] and "lut=" in texts[0]
    assert a.dtype == torch.uint8 and np.array_equal(a.numpy(), table) and np.array_equal(b.numpy(), table)
    assert "NOT OpenCV" in Pm.jet_lut.__doc__


def test_frame_reader_checks_its_arguments():
    from texgs import present as Pm
    for exc, pattern, args in [(TypeError, "capacity must be an int", (2.0, 4, 4)), (TypeError, "H must be an int", (2, "4", 4)),
                               (TypeError, "channels must be an int", (2, 4, 4, True)), (ValueError, "capacity must be at least 1", (0, 4, 4)),
                               (ValueError, r"H\*W must be in", (2, 0, 4)), (ValueError, r"H\*W must be in", (2, 65536, 32768)),
                               (ValueError, "channels must be 3 or 4", (2, 4, 4, 2))]:
        with pytest.raises(exc, match=pattern):
            Pm.FrameReader(*args)
    r = Pm.FrameReader(2, 4, 5)
    assert len(r) == 0 and list(r.drain()) == []
    with pytest.raises(ValueError, match="the reader was made for 4x5"):
        r.submit("a", torch.zeros(3, 5, 4))
    with pytest.raises(ValueError, match="order must be"):
        r.submit("a", torch.zeros(3, 4, 5), order="x")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.submit("a", torch.zeros(3, 4, 5))
    assert len(r) == 0              # a refused frame took no slot
