"""-m gpu: the kernels of csrc/present.hip against the numpy float32 statement of tests/present_ref.py.  EVERY output byte and float
is equal -- bytes as bytes, floats as bit patterns -- with no tolerance anywhere.

Shapes, from the kernels' constants (include/texgs_present.h): a thread takes 4 pixels, a workgroup 1024 per pass, the grid is capped at
2048 workgroups.  So: 1x1 (a tail only), 7x9 (P = 63: odd, planes 1 and 2 misaligned, a 3-pixel tail), 33x65, 64x64 (P % 4 == 0: the
16-byte paths), P = 1023 / 1024 / 1025 (one workgroup's pass minus one, exactly, plus one), and 1449x1448 > 2048 x 1024 pixels (the
grid-stride loop runs twice for some workgroups).  The depth range has no second-stage limit: every workgroup of the colouring pass
loops over all partials (at most 2048); 513x513 gives 258 of them, more than the 256 threads of that loop's first pass."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import present_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (7, 9), (33, 65), (64, 64), (1, 1023), (32, 32), (25, 41)]
BIG = (1449, 1448)
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """A device tensor against a numpy array: shape, dtype and every bit"""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{bad.size} elements differ, the first at flat index {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}"


@pytest.fixture(autouse=True)
def _quiet():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


@pytest.mark.parametrize("H,W", SMALL + [BIG])
def test_frame_display_and_chw_equal_the_statement(H, W):
    from texgs import present as Pm
    img, alpha1 = R.make_image(3, H, W, seed=1), R.make_image(1, H, W, seed=5)
    norm, alpha = R.make_image(3, H, W, seed=4, affine=True), R.make_alpha(H, W)
    d_img, d_alpha, d_bg = dev(img), dev(alpha), dev(R.BACKGROUND)
    # retexture: clamp only; composite over a background; both orders, 3 and 4 channels
    same_bits(Pm.frame_u8(d_img), R.frame_u8(img))
    same_bits(Pm.frame_u8(d_img, alpha=d_alpha, background=d_bg), R.frame_u8(img, alpha, R.BACKGROUND))
    same_bits(Pm.frame_u8(d_img, alpha=d_alpha[None], background=[float(v) for v in R.BACKGROUND], order="bgr", channels=4),
              R.frame_u8(img, alpha, R.BACKGROUND, order="bgr", channels=4))
    same_bits(Pm.frame_u8(d_img, order="bgr"), R.frame_u8(img, order="bgr"))
    same_bits(Pm.frame_u8(d_img, alpha=d_alpha, channels=4), R.frame_u8(img, alpha, None, channels=4))          # background None: black
    same_bits(Pm.frame_u8(d_img, alpha=d_alpha > 0, background=d_bg), R.frame_u8(img, (alpha > 0).astype(R.F), R.BACKGROUND))   # a bool mask
    # one channel, broadcast
    same_bits(Pm.frame_u8(dev(alpha1), alpha=d_alpha, background=d_bg, order="bgr"), R.frame_u8(alpha1, alpha, R.BACKGROUND, order="bgr"))
    # the viewer's frame
    same_bits(Pm.display(d_img), R.hwc4(R.present_values(img)))
    same_bits(Pm.display(dev(norm), mode="norm"), R.hwc4(R.present_values(norm, affine=True)))
    same_bits(Pm.display(dev(alpha1), mode="alpha"), R.hwc4(R.present_values(alpha1)))
    same_bits(Pm.display(dev(alpha1[0]), mode="alpha"), R.hwc4(R.present_values(alpha1)))
    # TensorBoard's planes
    same_bits(Pm.to_chw01(d_img), R.present_values(img))
    same_bits(Pm.to_chw01(dev(norm), affine=True), R.present_values(norm, affine=True))
    same_bits(Pm.to_chw01(dev(alpha1)), R.present_values(alpha1))


@pytest.mark.parametrize("H,W", [(7, 9), (64, 64)])
def test_every_output_subset_and_out_reuse(H, W):
    """The C entry writes any non-empty subset of its three outputs; a buffer it is not given stays as it was, a buffer it is given is
    written whole (poisoned first), and `out=` is the tensor that comes back."""
    from texgs import present as Pm
    img, alpha = R.make_image(3, H, W, seed=8), R.make_alpha(H, W)
    v = R.present_values(img, alpha, R.BACKGROUND, composite=True)
    want = {"u8": R.u8_frame(R.quantise(v), 4, "bgr"), "hwc4": R.hwc4(v), "chw": v}
    d_img, d_alpha, d_bg = dev(img), dev(alpha), dev(R.BACKGROUND)
    for subset in range(1, 8):
        bufs = {"u8": torch.full((H, W, 4), 0xAB, dtype=torch.uint8, device=DEV),
                "hwc4": torch.full((H, W, 4), -7.0, dtype=torch.float32, device=DEV), "chw": torch.full((3, H, W), -7.0, dtype=torch.float32, device=DEV)}
        use = {k: (b if subset >> i & 1 else None) for i, (k, b) in enumerate(bufs.items())}
        Pm._present(d_img, 3, H, W, d_alpha, d_bg, Pm.COMPOSITE | Pm.SWAP_RB, out_u8=use["u8"], u8_channels=4, out_hwc4=use["hwc4"],
                    out_chw=use["chw"])
        for k, b in bufs.items():
            if use[k] is not None:
                same_bits(b, want[k])
            else:
                assert bool((b == (0xAB if k == "u8" else -7.0)).all()), (subset, k)
    out = torch.full((H, W, 3), 0xAB, dtype=torch.uint8, device=DEV)
    assert Pm.frame_u8(d_img, out=out) is out
    same_bits(out, R.frame_u8(img))
    assert Pm.frame_u8(d_img, alpha=d_alpha, background=d_bg, out=out) is out           # reused
    same_bits(out, R.frame_u8(img, alpha, R.BACKGROUND))
    out4 = torch.full((H, W, 4), -7.0, dtype=torch.float32, device=DEV)
    assert Pm.display(d_img, out=out4) is out4
    same_bits(out4, R.hwc4(R.present_values(img)))
    with pytest.raises(RuntimeError, match="no output requested"):
        Pm._present(d_img, 3, H, W, None, None, 0)


def test_a_nan_gives_byte_zero_and_changes_nothing_else():
    from texgs import present as Pm
    H, W = 33, 65
    img, alpha = R.make_image(3, H, W, seed=9), R.make_alpha(H, W)
    alpha[10, 20] = 1
    clean = Pm.frame_u8(dev(img), alpha=dev(alpha), background=dev(R.BACKGROUND)).cpu().numpy()
    img[1, 10, 20] = np.nan
    got = Pm.frame_u8(dev(img), alpha=dev(alpha), background=dev(R.BACKGROUND))
    same_bits(got, R.frame_u8(img, alpha, R.BACKGROUND))
    got = got.cpu().numpy()
    assert got[10, 20, 1] == 0
    clean[10, 20, 1] = 0
    assert np.array_equal(got, clean)
    f = Pm.to_chw01(dev(img)).cpu().numpy()
    assert np.isnan(f[1, 10, 20]) and np.isnan(f).sum() == 1                            # the clamp keeps it


def depth_masks(H, W):
    single = np.zeros((H, W), R.F)
    single[H // 2, W // 2] = 1
    return {"none": None, "ones": np.ones((H, W), R.F), "single": single, "fraction": np.where(R.make_alpha(H, W) > 0, R.F(0.25), R.F(0)),
            "zero": np.zeros((H, W), R.F)}


@pytest.mark.parametrize("H,W", SMALL + [(513, 513), BIG])
def test_depth_picture_equals_the_statement(H, W):
    from texgs import present as Pm
    lut = R.random_lut()
    d_lut = dev(lut)
    depth = R.make_depth(H, W, seed=2)
    d_depth = dev(depth)
    for name, m in depth_masks(H, W).items():
        if (H, W) == BIG and name not in ("none", "fraction"):
            continue
        rgb, (lo, hi) = R.depth_colour(depth, m, lut)
        d_m = None if m is None else dev(m)
        got, rng = Pm.depth_colour(d_depth, mask=d_m, lut=d_lut, return_range=True)
        same_bits(got, R.bytes_as_float(rgb))
        same_bits(rng, np.array([lo, hi], dtype=R.F))
        if m is not None and (m != 0).any():
            assert lo == depth[m != 0].min() and hi == depth[m != 0].max()               # numpy's masked min / max
        if name == "zero":
            assert rng.cpu().tolist() == [np.inf, -np.inf] and not got.any()
        same_bits(Pm.depth_colour(d_depth[None], mask=None if m is None else d_m[None], lut=lut, as_float=False), R.u8_frame(rgb))
        same_bits(Pm.display(d_depth, mode="depth", alpha=d_m, lut=d_lut), R.hwc4(R.bytes_as_float(rgb)))
        again, rng2 = Pm.depth_colour(d_depth, mask=d_m, lut=d_lut, return_range=True)   # two calls: the same bits
        assert torch.equal(again.view(torch.int32), got.view(torch.int32)) and torch.equal(rng2.view(torch.int32), rng.view(torch.int32))
    if (H, W) != BIG:                                                                    # a bool mask selects what its float did
        fraction = depth_masks(H, W)["fraction"]
        same_bits(Pm.depth_colour(d_depth, mask=dev(fraction) != 0, lut=d_lut), R.bytes_as_float(R.depth_colour(depth, fraction, lut)[0]))


def test_depth_near_ties_flat_and_the_default_table():
    from texgs import present as Pm
    lut = R.random_lut()
    d = R.near_tie_depth()
    rgb, (lo, hi) = R.depth_colour(d, None, lut)
    got, rng = Pm.depth_colour(dev(d), lut=dev(lut), return_range=True)
    same_bits(got, R.bytes_as_float(rgb))
    assert rng.cpu().tolist() == [0.0, 255.0] == [float(lo), float(hi)]
    flat = np.full((5, 7), 3.25, R.F)                                                    # hi == lo
    same_bits(Pm.depth_colour(dev(flat), lut=dev(lut), as_float=False), R.u8_frame(R.depth_colour(flat, None, lut)[0]))
    # no lut: the classic jet
    depth = R.make_depth(33, 65, seed=3)
    same_bits(Pm.depth_colour(dev(depth)), R.bytes_as_float(R.depth_colour(depth, None, Pm.jet_table())[0]))


@pytest.mark.parametrize("res", [1, 3, 16])
def test_cross_equals_the_statement_in_every_cell(res):
    from texgs import present as Pm
    tex = R.make_texture(res, seed=7)
    want = R.cross_u8(tex)
    out = torch.full((3 * res, 4 * res, 3), 0xAB, dtype=torch.uint8, device=DEV)         # poisoned: the empty cells must be written too
    assert Pm.cross_u8(dev(tex), out=out) is out
    same_bits(out, want)
    same_bits(Pm.cross_u8(dev(tex)), want)
    got = out.cpu().numpy()
    for cy in range(3):
        for cx in range(4):
            cell = got[cy * res:(cy + 1) * res, cx * res:(cx + 1) * res]
            if (cy, cx) in R.CROSS_CELLS:
                assert np.array_equal(cell, R.quantise(R.clamp01(tex[R.CROSS_CELLS[(cy, cx)]] * R.SH_C0 + R.F(0.5)))), (cy, cx)
            else:
                assert not cell.any(), (cy, cx)


def test_frame_reader_keeps_order_through_a_ring_of_two():
    from texgs import present as Pm
    H, W = 33, 65
    alpha = R.make_alpha(H, W)
    frames = [R.make_image(3, H, W, seed=20 + k) for k in range(5)]
    reader = Pm.FrameReader(2, H, W, channels=3)
    out = []
    for k, img in enumerate(frames):
        handed = reader.submit(f"view{k}", dev(img), alpha=dev(alpha), background=dev(R.BACKGROUND), order="bgr")
        assert len(handed) == (1 if k >= 2 else 0) and len(reader) == min(k + 1, 2)
        out += handed
    out += list(reader.drain())
    assert len(reader) == 0 and [tag for tag, _ in out] == [f"view{k}" for k in range(5)]
    for (tag, got), img in zip(out, frames):
        want = R.frame_u8(img, alpha, R.BACKGROUND, order="bgr")
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), tag
    assert len({id(a) for _, a in out}) == 5 and not any(np.shares_memory(out[0][1], a) for _, a in out[1:])
