"""-m "not gpu": the input stage (texgs/ingest.py, include/texgs_ingest.h) without a GPU.

* The numpy statement (tests/ingest_ref.py) equals Pillow byte for byte -- live when Pillow imports, against tests/golden/ingest.npz
  always -- and the reference's PILtoTorch / loadCam / Camera lines (recorded in the golden from CPU torch) bit for bit.
* Structure: the ctypes mirror against gcc's layout of the header's struct, the header as plain C99, the exports and their signatures
  against the prototypes, the C entries' refusals (they need no GPU), the build script's knowledge of the unit.
* texgs.ingest refuses by name before any launch; `resolution_for` against a table; the composite's statement against the numpy
  expression of dataset_readers.py."""
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
import ingest_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_ingest.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ingest.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ---- the statement is Pillow ----
@pytest.mark.parametrize("shape,size", R.HOST_CASES, ids=lambda v: "x".join(str(s) for s in v))
def test_statement_is_pillow_recorded(golden, shape, size):
    for kind in R.KINDS:
        img = R.noise(shape, R.case_seed(shape, size), kind)
        for name in R.FILTERS:
            want = golden[R.case_key(shape, size, name, kind)]
            got = R.resize(img, size, name)
            assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), (name, kind)


def test_statement_is_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    flt = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX}
    for shape, size in R.HOST_CASES:
        for kind in R.KINDS:
            img = R.noise(shape, R.case_seed(shape, size), kind)
            for name in R.FILTERS:
                assert np.array_equal(R.resize(img, size, name), np.array(Image.fromarray(img).resize(size, flt[name]))), (shape, size, name, kind)
    img = R.noise((40, 30, 3), 3)
    assert np.array_equal(np.array(Image.fromarray(img).resize((11, 17))), R.resize(img, (11, 17), "bicubic"))     # the default filter


def test_binary_images_reach_both_clamps():
    """The bicubic overshoot of a 0 / 255 image leaves [0, 255] on both sides before the clamp: the clamp is exercised"""
    img = R.noise((37, 53, 3), R.case_seed((37, 53, 3), (53, 90)), "binary").astype(np.int64)
    kk, b = R.coeffs(37, 90, "bicubic")
    lo = hi = 0
    for yy in range(90):
        ymin, n = b[yy]
        acc = ((1 << 21) + np.tensordot(kk[yy, :n].astype(np.int64), img[ymin:ymin + n], axes=(0, 0))) >> 22
        lo, hi = min(lo, int(acc.min())), max(hi, int(acc.max()))
    assert lo < 0 and hi > 255


def test_tables_shapes_and_the_host_side_ksize(lib_built):
    from texgs import ingest
    lib = ingest.entry()
    for inS, outS in R.TABLE_CASES:
        for f, name in enumerate(R.FILTERS):
            k = R.ksize_of(inS, outS, name)         # (beyond the limit the library answers 0: 97 -> 1, 2, 3 bicubic and 97 -> 1 bilinear)
            assert lib.texgs_resize_ksize(inS, outS, f) == (k if k <= R.MAX_KSIZE else 0), (inS, outS, name)
    assert sorted(R.refused_tables()) == [(97, 1, "bicubic"), (97, 1, "bilinear"), (97, 2, "bicubic"), (97, 3, "bicubic")]
    for inS, outS in [(97, 1), (97, 33), (97, 64), (64, 97), (1600, 533), (7, 7), (4160, 130)]:
        for name in R.FILTERS:
            kk, b = R.coeffs(inS, outS, name)
            assert kk.shape == (outS, R.ksize_of(inS, outS, name)) and (b[:, 1] >= 1).all() and (b[:, 1] <= kk.shape[1]).all()
            assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= inS).all() and (np.diff(b[:, 0]) >= 0).all()
            assert np.abs(kk.astype(np.int64).sum(1) - (1 << 22)).max() <= kk.shape[1]         # each row sums to 1 up to its roundings
    assert R.ksize_of(4160, 130, "bicubic") == 129 == ingest.MAX_KSIZE
    assert lib.texgs_resize_ksize(4161, 130, ingest.BICUBIC) == 0 and "ksize 131" in lib.texgs_last_error().decode()
    assert lib.texgs_resize_ksize(4161, 130, ingest.BILINEAR) == 67


def test_decode_statement_is_the_reference(golden):
    for shape, size in R.P2T_CASES:
        img = R.noise(shape, R.case_seed(shape, size), "noise")
        want = golden["p2t_" + R.case_key(shape, size, "default", "noise")]
        got = R.pil_to_torch(img, size)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, size)
    for name, (H, W), res, with_alpha, with_normal in R.CAMERA_CASES:
        image, alpha, normal = R.camera_inputs(H, W)
        o, m, n = R.camera_images(image, res, alpha if with_alpha else None, normal if with_normal else None)
        assert np.array_equal(o.view(np.uint32), golden[f"cam_{name}_original"].view(np.uint32)), name
        assert (m is None) == (not with_alpha) and (n is None) == (not with_normal)
        if m is not None:
            assert np.array_equal(m, golden[f"cam_{name}_mask"]) and 0 < m.mean() < 1, name          # the mask zeroes pixels, not all
            assert (o[:, m[0] == 0] == 0).all()
        if n is not None:
            assert np.array_equal(n.view(np.uint32), golden[f"cam_{name}_normal"].view(np.uint32)), name
            assert n.min() >= -1 and n.max() <= 1 and n.min() < 0 < n.max()


def test_composite_statement_is_the_loader(golden):
    rgba = R.composite_input()
    for tag, bg in (("bg0", [0, 0, 0]), ("bg1", [1, 1, 1])):
        got = R.composite(rgba, bg)
        assert np.array_equal(got, golden["composite_" + tag])
        norm_data = rgba / 255.0                                    # dataset_readers.py:223-225
        arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + np.array(bg) * (1 - norm_data[:, :, 3:4])
        assert np.array_equal(got, np.array(arr * 255.0, dtype=np.byte).view(np.uint8))
    # every (colour, alpha) pair: the np.byte cast of the loader, seen as uint8, is the truncation
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    full = np.stack([c, c, c, a], axis=-1)
    for bg in ([0, 0, 0], [1, 1, 1]):
        n = full / 255.0
        arr = n[:, :, :3] * n[:, :, 3:4] + np.array(bg) * (1 - n[:, :, 3:4])
        assert np.array_equal(R.composite(full, bg), np.array(arr * 255.0, dtype=np.byte).view(np.uint8))


# ---- structure ----
def test_struct_matches_c_layout(tmp_path):
    from texgs import ingest
    consts = {"TEXGS_INGEST_BICUBIC": ingest.BICUBIC, "TEXGS_INGEST_BILINEAR": ingest.BILINEAR, "TEXGS_INGEST_BOX": ingest.BOX,
              "TEXGS_INGEST_PRECISION_BITS": ingest.PRECISION_BITS, "TEXGS_INGEST_MAX_KSIZE": ingest.MAX_KSIZE,
              "TEXGS_INGEST_MAX_SIDE": ingest.MAX_SIDE, "TEXGS_INGEST_SIGNED": ingest.SIGNED}
    assert sorted(ingest.MIRRORS) == ["TexGSResize"]
    assert abi_check.layout_mismatches("texgs_ingest.h", ingest.MIRRORS, consts, tmp_path) == []


def test_header_is_plain_c99_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_ingest.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert "TEXGS_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert '#include "texgs_ingest.h"' in open(os.path.join(ROOT, "texture-gs_amd", "csrc", "ingest.hip")).read()


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib, ingest, present
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(ingest.SIGNATURES) == sorted(["texgs_resize_ksize", "texgs_resize_taps", "texgs_resize_temp_bytes",
                                                                   "texgs_resize_u8", "texgs_rgba_composite"])
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, ingest.SIGNATURES, ingest.MIRRORS) == []
    lib = ingest.entry()
    assert lib is _lib.load() and lib.texgs_resize_u8.argtypes == ingest.SIGNATURES["texgs_resize_u8"][1]
    # its own table: neither the one tests/test_abi.py pins to texgs.h nor the output stage's
    assert not any(n in _lib.SIGNATURES or n in present.SIGNATURES for n in protos) and not hasattr(_lib, "ResizeStruct")
    build = abi_check.build_knows_header(HDR)
    assert build.UNITS["ingest.hip"] == ["-ffp-contract=off"]


def test_c_entries_refuse_bad_arguments_before_any_launch(lib_built):
    """No GPU here: a call that got as far as a launch would fail with a HIP error instead of the cause named below."""
    from texgs import ingest
    lib = ingest.entry()
    buf = (C.c_float * 64)()            # stands in for every device buffer: nothing may read it
    b = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.texgs_last_error().decode()
    Rz = lambda **kw: ingest.ResizeStruct(**{**dict(src=b, mul=None, out_u8=b, out_chw=None, out_mask=None, src_height=8, src_width=8,
                                                    channels=3, height=4, width=4, filter=0, flags=0), **kw})
    big = 1 << 30
    for kw, cause in [(dict(channels=4), "channels = 4 (RGBA) is not supported"), (dict(channels=2), "channels must be 1 or 3, got 2"),
                      (dict(filter=3), "unknown filter 3"), (dict(filter=-1), "unknown filter -1"), (dict(width=0), "sizes must be positive"),
                      (dict(src_height=-2), "sizes must be positive"), (dict(src_width=16385), "16385 -> 4: an image side above 16384"),
                      (dict(height=16385), "8 -> 16385: an image side above 16384"),
                      (dict(src_width=4161, width=130), "width: 4161 -> 130 needs ksize 131"),
                      (dict(src_height=8001, height=125, filter=1), "height: 8001 -> 125 needs ksize 131"),
                      (dict(src=None), "NULL argument (src or temp)"), (dict(flags=2), "unknown bit in flags"),
                      (dict(out_u8=None), "no output requested"), (dict(mul=b), "mul is read with out_chw only"),
                      (dict(src=b + 1), "4-byte aligned"), (dict(out_u8=b + 2), "4-byte aligned"), (dict(out_mask=b + 3), "4-byte aligned"),
                      (dict(out_chw=b + 1), "4-byte aligned"), (dict(out_chw=b, mul=b + 2), "4-byte aligned")]:
        assert lib.texgs_resize_u8(C.byref(Rz(**kw)), b, big, None) != 0, kw
        assert cause in err(), (kw, err())
    assert lib.texgs_resize_u8(None, b, big, None) != 0 and "NULL" in err()
    assert lib.texgs_resize_u8(C.byref(Rz()), None, big, None) != 0 and "NULL argument" in err()
    assert lib.texgs_resize_u8(C.byref(Rz()), b + 2, big, None) != 0 and "4-byte aligned" in err()
    need = lib.texgs_resize_temp_bytes(8, 8, 3, 4, 4, 0)
    # both passes (8 -> 4 bicubic is ksize 9): two tables of 9 x 4 taps and 4 bounds pairs, and 8 rows of 12 bytes
    assert need == 2 * (9 * 4 * 4 + 4 * 8) + 8 * 12
    assert lib.texgs_resize_u8(C.byref(Rz()), b, need - 1, None) != 0 and "temp is smaller" in err()
    assert lib.texgs_resize_temp_bytes(8, 8, 3, 8, 8, 0) == 4 and lib.texgs_resize_temp_bytes(8, 8, 3, 8, 4, 0) == 9 * 4 * 4 + 4 * 8
    assert lib.texgs_resize_temp_bytes(8, 7, 1, 4, 5, 2) == (3 * 5 * 4 + 5 * 8) + (3 * 4 * 4 + 4 * 8) + 8 * 8
    for args in [(8, 8, 4, 4, 4, 0), (8, 8, 3, 4, 4, 5), (0, 8, 3, 4, 4, 0), (8, 8, 3, 4, 16385, 0), (4161, 8, 3, 130, 4, 0)]:
        assert lib.texgs_resize_temp_bytes(*args) == 0, args
    for args, cause in [((0, 4, 0, b, b), "sizes must be positive"), ((8, 4, 7, b, b), "unknown filter 7"), ((16385, 4, 1, b, b), "above 16384"),
                        ((4161, 130, 0, b, b), "ksize 131"), ((8, 4, 0, None, b), "NULL argument"), ((8, 4, 0, b, None), "NULL argument"),
                        ((8, 4, 0, b + 2, b), "4-byte aligned")]:
        assert lib.texgs_resize_taps(*args, None) != 0, args
        assert cause in err(), (args, err())
    for args, cause in [((b, b, 0, 4, 0.0, 0.0, 0.0), "must be positive"), ((b, b, 4, 16385, 0.0, 0.0, 0.0), "above 16384"),
                        ((None, b, 4, 4, 0.0, 0.0, 0.0), "NULL argument"), ((b, None, 4, 4, 0.0, 0.0, 0.0), "NULL argument"),
                        ((b + 1, b, 4, 4, 0.0, 0.0, 0.0), "4-byte aligned"), ((b, b, 4, 4, 0.0, 1.5, 0.0), "background must lie in [0, 1]"),
                        ((b, b, 4, 4, float("nan"), 0.0, 0.0), "background must lie in [0, 1]"), ((b, b, 4, 4, 0.0, 0.0, -0.1), "background")]:
        assert lib.texgs_rgba_composite(*args, None) != 0, args
        assert cause in err(), (args, err())


# ---- texgs.ingest refuses by name, before any launch ----
def test_every_refusal_has_its_name():
    from texgs import ingest as I
    img = torch.zeros(8, 9, 3, dtype=torch.uint8)
    arr = np.zeros((8, 9, 3), np.uint8)
    bad = [
        (NotImplementedError, "4 channels", lambda: I.resize_u8(torch.zeros(8, 9, 4, dtype=torch.uint8), (4, 4))),
        (NotImplementedError, "4 channels", lambda: I.pil_to_torch(np.zeros((8, 9, 4), np.uint8), (4, 4))),
        (NotImplementedError, "filter 'lanczos' is not built", lambda: I.resize_u8(img, (4, 4), filter="lanczos")),
        (NotImplementedError, "filter 0 is not built", lambda: I.resize_u8(img, (4, 4), filter=0)),
        (NotImplementedError, "box=", lambda: I.resize_u8(img, (4, 4), box=(0, 0, 4, 4))),
        (NotImplementedError, "reducing_gap=", lambda: I.resize_u8(img, (4, 4), reducing_gap=2.0)),
        (ValueError, "img must be a torch.Tensor", lambda: I.resize_u8(arr, (4, 4))),
        (ValueError, "img must be torch.uint8", lambda: I.resize_u8(img.float(), (4, 4))),
        (ValueError, r"img must be \[H,W\] or \[H,W,C\]", lambda: I.resize_u8(torch.zeros(8, dtype=torch.uint8), (4, 4))),
        (ValueError, "img must have 1 or 3 channels, got 2", lambda: I.resize_u8(torch.zeros(8, 9, 2, dtype=torch.uint8), (4, 4))),
        (ValueError, "img must not be empty", lambda: I.resize_u8(torch.zeros(0, 9, 3, dtype=torch.uint8), (4, 4))),
        (ValueError, "img must be contiguous", lambda: I.resize_u8(torch.zeros(9, 8, 3, dtype=torch.uint8).transpose(0, 1), (4, 4))),
        (ValueError, r"size must be \(width, height\)", lambda: I.resize_u8(img, 4)),
        (ValueError, "size must hold two ints", lambda: I.resize_u8(img, (4.0, 4))),
        (ValueError, "size must be positive", lambda: I.resize_u8(img, (0, 4))),
        (ValueError, "an image side above 16384", lambda: I.resize_u8(img, (16385, 4))),
        (ValueError, "out must be a contiguous torch.uint8", lambda: I.resize_u8(img, (4, 5), out=torch.zeros(4, 5, 3, dtype=torch.uint8))),
        (ValueError, "out must be a contiguous torch.uint8", lambda: I.resize_u8(img, (4, 5), out=torch.zeros(5, 4, 3))),
        (ValueError, "no CPU fallback", lambda: I.resize_u8(img, (4, 4))),
        (ValueError, "image must be uint8", lambda: I.pil_to_torch(arr.astype(np.float32), (4, 4))),
        (ValueError, "image must be a PIL image", lambda: I.pil_to_torch([[1, 2]], (4, 4))),
        (ValueError, "no CPU fallback", lambda: I.pil_to_torch(arr, (4, 4), device="cpu")),
        (ValueError, r"image must be \[H,W,3\]", lambda: I.camera_images(arr[:, :, 0], (4, 4))),
        (ValueError, r"normal must be \[H,W,3\]", lambda: I.camera_images(arr, (4, 4), normal=arr[:, :, 0])),
        (ValueError, "alpha must be uint8", lambda: I.camera_images(arr, (4, 4), alpha=arr.astype(np.int32))),
        (ValueError, "no CPU fallback", lambda: I.camera_images(arr, (4, 4), device="cpu")),
        (ValueError, r"rgba must be \[H,W,4\]", lambda: I.composite_rgba_u8(img, [0, 0, 0])),
        (ValueError, "rgba must be torch.uint8", lambda: I.composite_rgba_u8(torch.zeros(4, 4, 4), [0, 0, 0])),
        (ValueError, "background must hold 3 values in", lambda: I.composite_rgba_u8(torch.zeros(4, 4, 4, dtype=torch.uint8), [0, 0])),
        (ValueError, "background must hold 3 values in", lambda: I.composite_rgba_u8(torch.zeros(4, 4, 4, dtype=torch.uint8), [0, 2, 0])),
        (ValueError, "background must be a sequence", lambda: I.composite_rgba_u8(torch.zeros(4, 4, 4, dtype=torch.uint8), 1.0)),
        (ValueError, "no CPU fallback", lambda: I.composite_rgba_u8(torch.zeros(4, 4, 4, dtype=torch.uint8), [0, 0, 0])),
        (ValueError, "capacity must be an int", lambda: I.ViewUploader(2.0, 4, 4)),
        (ValueError, "capacity must be at least 1", lambda: I.ViewUploader(0, 4, 4)),
        (ValueError, "max_h and max_w must be in", lambda: I.ViewUploader(2, 0, 4)),
        (ValueError, "no CPU fallback", lambda: I.ViewUploader(2, 4, 4, device="cpu")),
        (ValueError, "no CPU fallback", lambda: I.resize_taps(8, 4, device="cpu")),
        (NotImplementedError, "filter 'hamming'", lambda: I.resize_taps(8, 4, "hamming")),
    ]
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()


def test_limits_are_refused_by_value(lib_built):
    from texgs import ingest as I
    wide = torch.zeros(1, 4161, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="4161 -> 130 needs ksize 131"):
        I.resize_u8(wide, (130, 1))
    with pytest.raises(ValueError, match="ksize 131"):
        I.resize_taps(4161, 130)
    with pytest.raises(ValueError, match="an image side above 16384"):
        I.resize_u8(torch.zeros(1, 16385, dtype=torch.uint8), (4, 1))
    up = I.ViewUploader(2, 8, 9)
    assert len(up) == 0 and list(up.drain()) == []
    with pytest.raises(ValueError, match="made for at most 8x9"):
        up.submit("a", np.zeros((9, 9, 3), np.uint8), (4, 4))
    assert len(up) == 0


def test_resolution_for_is_loadcam():
    from texgs.ingest import resolution_for
    table = [((1600, 1200, 1), (1600, 1200)), ((1600, 1200, 2), (800, 600)), ((1601, 1201, 2), (800, 600)),      # 800.5 -> 800, 600.5 -> 600
             ((1603, 1203, 2), (802, 602)),                                                                        # 801.5 -> 802, 601.5 -> 602
             ((1001, 999, 4), (250, 250)), ((1002, 998, 4), (250, 250)),                                           # 250.5 -> 250, 249.5 -> 250
             ((1006, 1010, 4), (252, 252)),                                                                        # 251.5 -> 252, 252.5 -> 252
             ((100, 60, 8), (12, 8)),                                                                              # 12.5 -> 12, 7.5 -> 8
             ((1600, 1200, -1), (1600, 1200)), ((800, 800, -1), (800, 800)), ((3200, 2400, -1), (1600, 1200)),
             ((1601, 1200, -1), (1599, 1199)),              # 1601 / (1601 / 1600) is 1599.99... in doubles: the reference's int() gives 1599
             ((4032, 3024, -1), (1600, 1200)),
             ((1600, 1200, 400), (400, 300)), ((1000, 750, 333), (333, 249)), ((1920, 1080, 640.0), (640, 360))]
    for (w, h, r), want in table:
        assert resolution_for(w, h, r) == want, (w, h, r)
    assert resolution_for(1600, 1200, 2, 2.0) == (400, 300) and resolution_for(1602, 1202, 2, 2.0) == (400, 300)      # 400.5, 300.5
    assert resolution_for(3200, 2400, -1, 2.0) == (800, 600) and resolution_for(1000, 500, 500, 4.0) == (125, 62)
    assert all(isinstance(v, int) for v in resolution_for(1601, 1201, 2))
