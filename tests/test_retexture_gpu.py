"""-m gpu: the retexture stage on the device (texgs/retexture.py, csrc/retexture.hip) against its numpy statement
(tests/retexture_ref.py).

* The cross path is a bit-exact contract: every mode and both channel orders at six (r, R) pairs, the golden case against the
  reference's own results, in place, inside guarded allocations, at byte offsets past 2^31, and from a PNG file against the host path.
* The lat-long path is fp64 geometry with fp32 blending: its error against the float64 statement is at most 4 x the error of the
  mixed-precision statement (the project's standing bound); the wrap at the seam and the orientation through `cubetex.sphere_map`.
* Refusals that need a device, and the returned tensor through the rasterizer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retexture_ref as R  # noqa: E402
from texgs import retexture as RT  # noqa: E402
from texgs import texture_io as TIO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_io.npz"))
PAIRS = [(12, 12), (7, 5), (3, 8), (1, 4), (5, 33), (40, 17)]          # (r, R); 6 * 33^2 = 6534 = 25 workgroups of 256 + 134: a tail
JUNK = 0x7FC5A5A5           # a NaN with a payload: a guard word nothing may write
PARITY_FACTOR = 4.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---- 1. the cross path, bit for bit ----
@pytest.mark.parametrize("r,R_", PAIRS)
def test_cross_has_the_bits_of_the_statement(r, R_):
    cross, tex = R.hard_cross(r, seed=100 + r), R.hard_texture(R_, seed=200 + R_)
    faces = R.cross_new_u8(cross, R_)
    sums = faces.astype(np.int64).sum(-1)
    assert (sums == 0).any() or r == 1          # black texels inside used cells: x/0 and 0/0 in mode 2 (r = 1: every texel is a blend)
    assert (sums == 2).any() and (sums == 3).any()              # the two sides of mode 3's 0.01
    d_tex = dev(tex)
    d_cross = {"rgb": dev(cross), "bgr": dev(cross[..., ::-1])}
    for mode in R.MODES:
        want = R.retexture_cross(tex, cross, mode)
        for order in ("rgb", "bgr"):
            got = RT.retexture_cross_u8(d_tex, d_cross[order], mode=mode, order=order)
            assert got.dtype == torch.float32 and tuple(got.shape) == (6, R_, R_, 3) and not got.requires_grad
            assert R.same_class_and_bits(host(got), want), (mode, order)
    if r < R_:                      # a bgr cross read as rgb differs: the order is not ignored
        assert not R.same_class_and_bits(host(RT.retexture_cross_u8(d_tex, d_cross["bgr"], mode=-1, order="rgb")), R.retexture_cross(tex, cross, -1))
    assert torch.equal(d_tex, dev(tex))         # the input is left alone out of place


@pytest.mark.parametrize("mode", R.MODES)
def test_golden_case_has_the_bits_of_the_reference(mode):
    got = RT.retexture_cross_u8(dev(G["texture0"]), dev(G["cross_u8"]), mode=mode)
    assert R.same_class_and_bits(host(got), G[f"change_texture_m{mode + 1}"])


# ---- 2. in place, twice, inside guards ----
def guarded(shape, guard_words=4096):
    """A float32 tensor of `shape` inside one allocation, JUNK words either side -> (tensor, check)"""
    n = int(np.prod(shape))
    pad = (-n) % 4          # keeps the tensor 16-byte aligned behind the first guard
    flat = torch.full((2 * guard_words + n + pad,), JUNK, dtype=torch.int32, device=DEV)
    t = flat[guard_words:guard_words + n].view(torch.float32).view(*shape)

    def check():
        assert bool((flat[:guard_words] == JUNK).all()) and bool((flat[guard_words + n:] == JUNK).all()), "a guard word was written"
    return t, check


@pytest.mark.parametrize("r,R_", [(5, 33), (12, 12), (3, 8)])
def test_in_place_and_twice_and_inside_guards(r, R_):
    cross, tex = R.hard_cross(r, seed=100 + r), R.hard_texture(R_, seed=200 + R_)
    d_cross = dev(cross)
    for mode in R.MODES:
        first = RT.retexture_cross_u8(dev(tex), d_cross, mode=mode)
        again = RT.retexture_cross_u8(dev(tex), d_cross, mode=mode)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32))
        t, check = guarded((6, R_, R_, 3))
        t.copy_(dev(tex))
        back = RT.retexture_cross_u8(t, d_cross, mode=mode, out=t)
        assert back is t and torch.equal(t.view(torch.int32), first.view(torch.int32)), mode
        check()
        # a tensor that is only 4-byte aligned takes the dword path: same bits, same guards
        flat = torch.full((8192 + tex.size,), JUNK, dtype=torch.int32, device=DEV)
        u = flat[4097:4097 + tex.size].view(torch.float32).view(6, R_, R_, 3)
        assert u.data_ptr() % 16 == 4
        u.copy_(dev(tex))
        RT.retexture_cross_u8(u, d_cross, mode=mode, out=u)
        assert torch.equal(u.view(torch.int32), first.view(torch.int32)), mode
        assert bool((flat[:4097] == JUNK).all()) and bool((flat[4097 + tex.size:] == JUNK).all())
    # a parameter that requires grad is accepted, detached, and may be its own output
    p = torch.nn.Parameter(dev(tex))
    out = RT.retexture_cross_u8(p, d_cross, mode=1)
    assert not out.requires_grad and out.grad_fn is None
    with pytest.raises(ValueError, match="out overlaps texture_sh0"):
        buf = torch.zeros(tex.size + 3, device=DEV)
        RT.retexture_cross_u8(buf[:tex.size].view(6, R_, R_, 3), d_cross, out=buf[3:].view(6, R_, R_, 3))


# ---- 3. offsets past 2^31 bytes ----
def test_offsets_past_two_gib_in_place():
    """R = 5462: 6 R^2 12 bytes = 2 148 001 728.  One tensor, filled on the device, retextured in place; the statement is evaluated
    at the listed texels only (the 4 x 4 corner blocks of all six faces and the last 64 texels of face 5), and only they are read."""
    R_, r, mode, order = 5462, 8, 3, "bgr"
    assert 6 * R_ * R_ * 12 > 2 ** 31
    cross = R.hard_cross(r, seed=31)
    t, check = guarded((6, R_, R_, 3))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    t.uniform_(-2.5, 2.5, generator=gen)
    c = np.r_[0:4, R_ - 4:R_]
    fyx = np.array([(f, y, x) for f in range(6) for y in c for x in c if (y < 4 or y >= R_ - 4) and (x < 4 or x >= R_ - 4)], np.int64)
    last = np.stack([np.full(64, 5), np.full(64, R_ - 1), np.arange(R_ - 64, R_)], -1)
    fyx = np.concatenate([fyx, last])
    assert len(fyx) == 6 * 64 + 64
    idx = torch.from_numpy((fyx[:, 0] * R_ + fyx[:, 1]) * R_ + fyx[:, 2]).to(DEV)
    rows = t.view(-1, 3)
    assert int(idx.max()) * 12 > 2 ** 31
    old = host(rows[idx])
    RT.retexture_cross_u8(t, dev(cross), mode=mode, order=order, out=t)
    got = host(rows[idx])
    check()
    want = R.retexture_cross_at(old, cross, R_, mode, order, fyx)
    assert R.same_class_and_bits(got, want)
    assert not np.array_equal(got, old)
    del t, rows
    torch.cuda.empty_cache()


# ---- 4. from a PNG file ----
@pytest.mark.parametrize("mode", [0, 3])
def test_png_equals_the_host_path_bit_for_bit(tmp_path, mode):
    from PIL import Image
    r, R_ = 10, 24
    path = str(tmp_path / "cross.png")
    Image.fromarray(R.hard_cross(r, seed=77), "RGB").save(path)
    tex = R.hard_texture(R_, seed=78)
    want = TIO.change_texture(torch.from_numpy(tex), TIO.load_cross_png(path, R_), mode).numpy()
    got = RT.retexture_png(dev(tex), path, mode=mode)
    assert R.same_class_and_bits(host(got), want)
    bad = str(tmp_path / "bad.png")
    Image.fromarray(np.zeros((6, 9, 3), np.uint8), "RGB").save(bad)
    with pytest.raises(ValueError, match="a cubemap cross must be 3r x 4r pixels"):
        RT.retexture_png(dev(tex), bad)


# ---- 5. the lat-long path ----
LATLONG_CASES = [(4, 8, 3), (16, 32, 8), (5, 7, 6), (64, 128, 33)]      # (h, w, R)


@pytest.mark.parametrize("h,w,R_", LATLONG_CASES)
@pytest.mark.parametrize("u8", [False, True])
def test_latlong_within_four_times_the_statements_own_error(h, w, R_, u8):
    rng = np.random.default_rng(1000 * h + R_)
    pic = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if u8 else rng.random((h, w, 3)).astype(F)
    tex = rng.uniform(-1.5, 1.5, (6, R_, R_, 3)).astype(F)
    d_pic, d_tex = dev(pic), dev(tex)
    for mode in (-1, 0):
        truth = R.latlong_f64(pic, R_, tex, mode)
        e_ref = float(np.abs(R.latlong_mixed(pic, R_, tex, mode).astype(np.float64) - truth).max())
        got = RT.retexture_latlong(d_pic, texture_sh0=None if mode == -1 else d_tex, R=R_, mode=mode)
        assert got.dtype == torch.float32 and tuple(got.shape) == (6, R_, R_, 3)
        e_dev = float(np.abs(host(got).astype(np.float64) - truth).max())
        print(f"latlong {h}x{w} -> R={R_} u8={u8} mode={mode}: device {e_dev:.3e}, mixed statement {e_ref:.3e}")
        assert e_ref > 0 and e_dev <= PARITY_FACTOR * e_ref, (mode, e_dev, e_ref)
    # in place over the old texture, and R taken from it
    want = RT.retexture_latlong(d_pic, texture_sh0=d_tex, mode=0)
    t = d_tex.clone()
    assert RT.retexture_latlong(d_pic, texture_sh0=t, mode=0, out=t) is t and torch.equal(t.view(torch.int32), want.view(torch.int32))


def test_latlong_wraps_at_the_seam_on_the_device():
    R_, h, w = 64, 16, 32
    at, wx = R.seam_texels(R_, h, w)
    got = host(RT.retexture_latlong(dev(R.seam_picture(h, w)), R=R_))[R.SEAM_FACE][at[:, 0], at[:, 1]].astype(np.float64) * 0.28209479177387814 + 0.5
    np.testing.assert_allclose(got, np.repeat(wx[:, None], 3, 1), rtol=0, atol=1e-6)     # the blend of the last and the first column
    assert ((wx > 0.05) & (wx < 0.95)).any()


def test_latlong_orientation_round_trip_through_sphere_map():
    from texgs import cubetex
    rgb = np.broadcast_to(R.FACE_COLOURS[:, None, None, :], (6, 16, 16, 3))
    tex = dev(((rgb - F(0.5)) / R.C0).astype(F))
    pic = cubetex.sphere_map(tex, (256, 512))
    back = host(RT.retexture_latlong(pic, R=8)).astype(np.float64) * 0.28209479177387814 + 0.5
    for f in range(6):
        np.testing.assert_allclose(back[f, 2:6, 2:6], np.broadcast_to(R.FACE_COLOURS[f], (4, 4, 3)), rtol=0, atol=1e-6, err_msg=str(f))


# ---- 6. refusals that need a device ----
def test_refusals_by_name():
    tex, cross, pic = torch.zeros(6, 4, 4, 3, device=DEV), torch.zeros(6, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(4, 8, 3, device=DEV)
    bad = [
        (RuntimeError, r"texgs\.retexture\.retexture_cross_u8: cross_u8 is on cpu", lambda: RT.retexture_cross_u8(tex, cross.cpu())),
        (RuntimeError, r"texgs\.retexture\.retexture_cross_u8: texture_sh0 is on cpu", lambda: RT.retexture_cross_u8(tex.cpu(), cross)),
        (RuntimeError, r"texgs\.retexture\.retexture_cross_u8: out is on cpu", lambda: RT.retexture_cross_u8(tex, cross, out=tex.cpu())),
        (RuntimeError, r"texgs\.retexture\.retexture_latlong: latlong is on cpu", lambda: RT.retexture_latlong(pic.cpu(), texture_sh0=tex, mode=0)),
        (RuntimeError, r"texgs\.retexture\.retexture_png: texture_sh0 is on cpu", lambda: RT.retexture_png(tex.cpu(), "nothing.png")),
        (ValueError, "cross_u8 must be torch.uint8", lambda: RT.retexture_cross_u8(tex, cross.float())),
        (ValueError, "texture_sh0 must be torch.float32", lambda: RT.retexture_cross_u8(tex.half(), cross)),
        (ValueError, "latlong must be torch.float32 or torch.uint8", lambda: RT.retexture_latlong(pic.half(), R=4)),
        (ValueError, "texture_sh0 must be contiguous", lambda: RT.retexture_cross_u8(torch.zeros(6, 4, 4, 6, device=DEV)[..., ::2], cross)),
        (ValueError, "cross_u8 must be contiguous", lambda: RT.retexture_cross_u8(tex, torch.zeros(6, 8, 6, dtype=torch.uint8, device=DEV)[..., ::2])),
        (ValueError, "latlong must be contiguous", lambda: RT.retexture_latlong(torch.zeros(8, 4, 3, device=DEV).transpose(0, 1), R=4)),
        (ValueError, r"a cubemap cross must be \[3r,4r,3\]", lambda: RT.retexture_cross_u8(tex, torch.zeros(6, 9, 3, dtype=torch.uint8, device=DEV))),
        (ValueError, r"out must be \[6,4,4,3\]", lambda: RT.retexture_cross_u8(tex, cross, out=torch.zeros(6, 5, 5, 3, device=DEV))),
        (ValueError, "mismatched resolutions", lambda: RT.retexture_latlong(pic, R=5, texture_sh0=tex, mode=1)),
        (ValueError, "texture_sh0 is needed by mode 2", lambda: RT.retexture_latlong(pic, R=4, mode=2)),
        (ValueError, "mode must be -1, 0, 1, 2 or 3", lambda: RT.retexture_cross_u8(tex, cross, mode=4)),
        (ValueError, "order must be 'rgb' or 'bgr'", lambda: RT.retexture_cross_u8(tex, cross, order="RGB")),
    ]
    before = tex.clone()
    for exc, pattern, call in bad:
        with pytest.raises(exc, match=pattern):
            call()
    assert torch.equal(tex, before)


# ---- 7. the returned tensor is taken as it is ----
def test_the_returned_texture_renders_like_the_host_paths():
    import helpers as Hh
    from texgs import synth
    from texgs.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    scene = synth.make_scene(2000, 32, seed=21, scale_mean=0.05)
    cam = synth.fibonacci_cameras(4, 64, 64)[1]
    d = torch.device(DEV)
    st = Hh.settings_for(cam, 2, torch.tensor([0.1, 0.0, 0.2]), device=d, cls=GaussianRasterizationSettings)
    cross = R.hard_cross(20, seed=3)
    old = scene.texture.contiguous().float()
    assert tuple(old.shape) == (6, 32, 32, 3)
    host_tex = TIO.change_texture(old, torch.from_numpy(TIO.resize_bilinear_u8(cross, 96, 128).astype(F) / F(255.0)), 0)
    dev_tex = RT.retexture_cross_u8(old.to(d), dev(cross), mode=0)
    assert R.same_class_and_bits(host(dev_tex), host_tex.numpy())
    t_ = lambda v: v.to(d)
    m3 = t_(scene.means3D)

    def render(texture):
        with torch.no_grad():
            out = GaussianRasterizer(raster_settings=st)(means3D=m3, means2D=torch.zeros_like(m3), shs=t_(scene.shs), opacities=t_(scene.opacities),
                                                         scales=t_(scene.scales), rotations=t_(scene.rotations), uvs=t_(scene.uvs),
                                                         gradient_uvs=t_(scene.gradient_uvs), texture=texture, extra_attrs=None)
        return out[0]
    a, b, c = render(dev_tex), render(host_tex.to(d)), render(old.to(d))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a, c) and float(a.abs().max()) > 0
    torch.cuda.synchronize()
