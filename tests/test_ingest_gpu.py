"""-m gpu: the input stage on the device (texgs/ingest.py, csrc/ingest.hip) against its numpy statement (tests/ingest_ref.py) and
against what Pillow and the reference's lines returned (tests/golden/ingest.npz).  Every comparison is exact: bytes with
array_equal, floats as their 32 bits.  Needs neither Pillow nor the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def I(lib_built):
    from texgs import ingest
    return ingest


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the tables ----
@pytest.mark.parametrize("name", R.FILTERS)
def test_taps_equal_the_statement(I, name):
    refused = []
    for inS, outS in R.TABLE_CASES:
        if R.ksize_of(inS, outS, name) > R.MAX_KSIZE:       # 97 -> 1, 2, 3 bicubic, 97 -> 1 bilinear: refused by name (the limit is 129)
            with pytest.raises(ValueError, match=f"{inS} -> {outS} needs ksize {R.ksize_of(inS, outS, name)}"):
                I.resize_taps(inS, outS, name)
            refused.append((inS, outS, name))
            continue
        taps, bounds = I.resize_taps(inS, outS, name)
        kk, b = R.coeffs(inS, outS, name)
        assert taps.dtype == torch.int32 and tuple(taps.shape) == kk.shape
        assert np.array_equal(bounds.cpu().numpy(), b), (inS, outS)
        assert np.array_equal(taps.cpu().numpy(), kk), (inS, outS)
    assert refused == [c for c in R.refused_tables() if c[2] == name]
    if name == "bicubic":
        assert R.ksize_of(4160, 130, name) == 129 and I.resize_taps(4160, 130, name)[0].shape[1] == 129
        with pytest.raises(ValueError, match="4161 -> 130 needs ksize 131"):       # one size beyond
            I.resize_taps(4161, 130, name)


# ---- the resample ----
@pytest.mark.parametrize("shape,size", R.GPU_CASES, ids=lambda v: "x".join(str(s) for s in v))
def test_resize_equals_pillow_and_the_statement(I, golden, shape, size):
    ran = 0
    for kind in R.KINDS:
        img = R.noise(shape, R.case_seed(shape, size), kind)
        src = dev(img)
        for name in R.FILTERS:
            if not R.fits(shape, size, name):           # e.g. 90 x 75 -> 1 x 1, bicubic and bilinear: beyond the limit, refused by name
                with pytest.raises(ValueError, match="needs ksize"):
                    I.resize_u8(src, size, name)
                continue
            got = I.resize_u8(src, size, name)
            want = golden[R.case_key(shape, size, name, kind)]
            assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (name, kind)
            assert np.array_equal(want, R.resize(img, size, name))
            ran += 1
    assert ran == 2 * {(90, 75, 3): 1, (2, 3000, 3): 2, (1, 16384): 1}.get(shape, 3)      # the filters within the limit, both kinds


@pytest.fixture(scope="module")
def big():
    img = R.noise((1200, 1600, 3), 11)
    return img, R.resize(img, (800, 600))


def test_resize_1200x1600_to_600x800(I, big):
    img, want = big
    got = I.resize_u8(dev(img), (800, 600))
    assert np.array_equal(got.cpu().numpy(), want)


def test_out_unaligned_rows_and_twice(I):
    # rows of 53 * 3 = 159 and 23 * 3 = 69 bytes: no row but the first starts on a dword; one channel: rows of 29 -> 7 bytes
    for shape, size in [((37, 53, 3), (23, 11)), ((31, 29), (7, 5)), ((37, 53, 3), (53, 11)), ((37, 53, 3), (23, 37)), ((6, 1, 3), (1, 3))]:
        img = R.noise(shape, 9)
        want = R.resize(img, size)
        src = dev(img)
        out = torch.full(want.shape, 0xAB, dtype=torch.uint8, device="cuda")
        back = I.resize_u8(src, size, out=out)
        assert back is out and np.array_equal(out.cpu().numpy(), want), (shape, size)
        again = I.resize_u8(src, size)
        assert np.array_equal(again.cpu().numpy(), want), (shape, size)
        assert np.array_equal(src.cpu().numpy(), img)               # the source is only read
    # an output inside a larger buffer: nothing around it is written
    img = R.noise((37, 53, 3), 9)
    want = R.resize(img, (23, 11))
    n = want.size
    pad = torch.full((n + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    I.resize_u8(dev(img), (23, 11), out=pad[32:32 + n].view(11, 23, 3))
    host = pad.cpu().numpy()
    assert np.array_equal(host[32:32 + n].reshape(want.shape), want) and (host[:32] == 0xCD).all() and (host[32 + n:] == 0xCD).all()


# ---- the decode, fused into the last pass ----
def test_pil_to_torch_is_the_reference(I, golden):
    for shape, size in R.P2T_CASES:
        img = R.noise(shape, R.case_seed(shape, size), "noise")
        want = golden["p2t_" + R.case_key(shape, size, "default", "noise")]
        for source in (img, torch.from_numpy(img), dev(img)):
            got = I.pil_to_torch(source, size)
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
            assert np.array_equal(bits(got), bits(want)), (shape, size)
    with pytest.raises(ValueError, match="needs ksize"):
        I.pil_to_torch(R.noise((90, 75, 3), 1), (1, 1))


@pytest.mark.parametrize("case", R.CAMERA_CASES, ids=lambda c: c[0])
def test_camera_images_are_the_reference(I, golden, case):
    """With and without alpha and normal; a mask that zeroes pixels; through both passes, each single pass (a skipped axis) and no
    resize at all"""
    name, (H, W), res, with_alpha, with_normal = case
    image, alpha, normal = R.camera_inputs(H, W)
    o, m, n = I.camera_images(image, res, alpha=alpha if with_alpha else None, normal=normal if with_normal else None)
    w, h = res
    assert tuple(o.shape) == (3, h, w) and np.array_equal(bits(o), bits(golden[f"cam_{name}_original"]))
    assert (m is None) == (not with_alpha) and (n is None) == (not with_normal)
    if with_alpha:
        assert tuple(m.shape) == (1, h, w) and np.array_equal(bits(m), bits(golden[f"cam_{name}_mask"]))
        assert 0 < float(m.mean()) < 1
    if with_normal:
        assert tuple(n.shape) == (3, h, w) and np.array_equal(bits(n), bits(golden[f"cam_{name}_normal"]))
    so, sm, sn = R.camera_images(image, res, alpha if with_alpha else None, normal if with_normal else None)
    assert np.array_equal(bits(o), bits(so))
    # from device bytes, and a one-channel alpha: the same tensors
    o2, m2, n2 = I.camera_images(dev(image), res, alpha=dev(alpha[:, :, 0]) if with_alpha else None, normal=dev(normal) if with_normal else None)
    assert np.array_equal(bits(o2), bits(o)) and (m2 is None or np.array_equal(bits(m2), bits(m))) and (n2 is None or np.array_equal(bits(n2), bits(n)))


def test_decode_at_the_big_size(I, big):
    img, want = big
    got = I.pil_to_torch(img, (800, 600))
    assert np.array_equal(bits(got), bits(R.decode(want)))


# ---- the composite ----
def test_composite_is_the_loader(I, golden):
    rgba = R.composite_input()
    assert rgba.shape == (33, 17, 4)
    src = dev(rgba)
    for tag, bg in (("bg0", [0, 0, 0]), ("bg1", [1, 1, 1])):
        got = I.composite_rgba_u8(src, bg)
        assert tuple(got.shape) == (33, 17, 3) and np.array_equal(got.cpu().numpy(), golden["composite_" + tag])
    bg = [0.25, 1.0, 0.1]
    out = torch.zeros(33, 17, 3, dtype=torch.uint8, device="cuda")
    assert I.composite_rgba_u8(src, bg, out=out) is out and np.array_equal(out.cpu().numpy(), R.composite(rgba, bg))
    one = R.noise((1, 3, 4), 5)                # fewer than 4 pixels: the partial quad
    assert np.array_equal(I.composite_rgba_u8(dev(one), bg).cpu().numpy(), R.composite(one, bg))


# ---- the upload ring ----
def test_view_uploader_keeps_order_and_slots(I):
    """5 views of two sizes through 2 slots: in order, equal to the direct calls -- which they would not be had a slot's bytes been
    overwritten before its kernels had read them -- and every slot still holds the bytes of the last view it staged."""
    views = []
    for i in range(5):
        H, W = ((37, 53), (24, 31))[i % 2]
        image, alpha, normal = R.camera_inputs(H, W, seed=20 + 3 * i)
        res = ((20, 13), (31, 12))[i % 2]
        views.append((f"view{i}", image, res, alpha if i != 3 else None, normal if i != 1 else None))
    up = I.ViewUploader(2, 37, 53)
    for tag, image, res, alpha, normal in views:
        assert up.submit(tag, image, res, alpha=alpha, normal=normal) is None
    assert len(up) == 5
    got = list(up.drain())
    assert len(up) == 0 and [t for t, _ in got] == [v[0] for v in views]
    for (tag, outs), (_, image, res, alpha, normal) in zip(got, views):
        want = I.camera_images(image, res, alpha=alpha, normal=normal)
        for a, b in zip(outs, want):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(bits(a), bits(b)), tag
    torch.cuda.synchronize()
    for slot, i in ((0, 4), (1, 3)):            # views 0, 2, 4 went through slot 0, views 1, 3 through slot 1
        image = views[i][1]
        for buf in (up._pinned[slot], up._dev[slot].cpu()):
            assert np.array_equal(buf[:image.size].numpy().reshape(image.shape), image), slot
