"""-m gpu: the kernels of csrc/surface.hip against the numpy statement of tests/surface_ref.py.  EVERY output is equal -- counts and
indices as integers, floats as bit patterns -- with no tolerance anywhere.

Shapes, from the kernels' constants (include/texgs_surface.h): a thread takes 4 pixels, a workgroup B = 1024, the scanning workgroup
S = 256 counts per pass.  So: 1x1; 1x(B-1), 1xB, 1x(B+1) (one workgroup minus one, exactly, plus one; B-1 and B+1 are no multiple of
4: a thread with a partial quad); 17x23 (P = 391, the golden map's size); (B+1)x3 (rows that start anywhere in a quad, four
workgroups); 513x512 (257 workgroups > S: the scan runs a second pass with a carry).  Masks: tests/surface_ref.py `masks`."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as R  # noqa: E402
from texgs import surface as _surface  # noqa: E402,F401  (the feature under test: without it this file fails at import)

pytestmark = pytest.mark.gpu

B, S = 1024, 256
SHAPES = [(1, 1), (1, B - 1), (1, B), (1, B + 1), (17, 23), (B + 1, 3), (513, 512)]
MASKS = ["none", "all", "first", "last", "alternate", "runs", "random", "special"]
DEV = "cuda:0"
POISON_F = np.float32(-7.5)
POISON_I = -77


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """A device tensor against a numpy array: shape, dtype and every bit.  A NaN must meet a NaN; its sign and payload are not
    compared (the host and the device make different default NaNs, and IEEE leaves that open)."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        nan = np.uint32(0x7FC00000)
        got = np.where(np.isnan(got), nan, np.ascontiguousarray(got).view(np.uint32))
        want = np.where(np.isnan(want), nan, np.ascontiguousarray(want).view(np.uint32))
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{bad.size} elements differ, the first at flat index {bad[0]}: {got.reshape(-1)[bad[0]]} != {want.reshape(-1)[bad[0]]}"


@functools.lru_cache(maxsize=None)
def scene(H, W):
    """Per shape, computed once and left unchanged: depth, camera, every pixel's point by the statement, the masks"""
    depth = R.make_depth(H, W, seed=H + W)
    proj, zfar, znear = R.camera(H, W, seed=H)
    world = R.world_points(depth, proj, zfar, znear)
    return depth, proj, zfar, znear, world, R.masks(H, W, B)


def expected(H, W, alpha, threshold=0.5):
    depth, proj, zfar, znear, world, _ = scene(H, W)
    a = alpha.reshape(-1)
    with np.errstate(invalid="ignore"):
        index = np.flatnonzero(a > np.float32(threshold)).astype(np.int64)
    rank = np.full(H * W, -1, np.int32)
    rank[index] = np.arange(index.size, dtype=np.int32)
    return dict(count=int(index.size), index=index, xyz=np.ascontiguousarray(world[index]), alpha=a[index].copy(), rank=rank)


def c_call(d_depth, d_alpha, d_proj, zfar, znear, H, W, threshold=0.5, temp=None, stream=None, outputs=("index", "alpha_sel", "rank")):
    """The C entry on poisoned buffers -> (count tensor, xyz, index, alpha_sel, rank) as device tensors (None where not asked for)"""
    from texgs import _lib, surface as Sm
    lib = Sm.entry()
    n = H * W
    xyz = torch.full((n, 3), float(POISON_F), dtype=torch.float32, device=DEV)
    index = torch.full((n,), POISON_I, dtype=torch.int64, device=DEV) if "index" in outputs else None
    asel = torch.full((n,), float(POISON_F), dtype=torch.float32, device=DEV) if "alpha_sel" in outputs else None
    rank = torch.full((n,), POISON_I, dtype=torch.int32, device=DEV) if "rank" in outputs else None
    count = torch.full((1,), POISON_I, dtype=torch.int32, device=DEV)
    nbytes = lib.texgs_surface_temp_bytes(H, W)
    if temp is None:
        temp = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    assert temp.numel() * 8 >= nbytes
    p = _lib.ptr
    st = Sm.SurfacePointsStruct(p(d_depth), p(d_alpha), p(d_proj), p(xyz), p(index), p(asel), p(rank), p(count), zfar, znear, threshold, H, W, n)
    s = torch.cuda.current_stream(DEV) if stream is None else stream
    _lib.call(lib.texgs_surface_points, C.byref(st), p(temp), temp.numel() * 8, s.cuda_stream)
    return count, xyz, index, asel, rank


def check_c_outputs(outs, want, n):
    count, xyz, index, asel, rank = outs
    M = want["count"]
    assert int(count.cpu()[0]) == M
    same_bits(xyz[:M], want["xyz"])
    same_bits(index[:M], want["index"])
    same_bits(asel[:M], want["alpha"])
    same_bits(rank, want["rank"])
    # rows at and past the count keep the poison
    assert bool((xyz[M:].view(torch.int32) == int(np.float32(POISON_F).view(np.int32))).all())
    assert bool((index[M:] == POISON_I).all()) and bool((asel[M:].view(torch.int32) == int(np.float32(POISON_F).view(np.int32))).all())


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_points_equal_the_statement(H, W, mask):
    from texgs import surface as Sm
    depth, proj, zfar, znear, world, masks = scene(H, W)
    alpha = masks[mask]
    want = expected(H, W, alpha)
    if mask == "all":
        assert want["count"] == H * W
    if mask in ("none",):
        assert want["count"] == 0
    d_depth, d_alpha, d_proj = dev(depth), dev(alpha), dev(proj)
    first = c_call(d_depth, d_alpha, d_proj, zfar, znear, H, W)
    check_c_outputs(first, want, H * W)
    # two calls give the same bytes
    again = c_call(d_depth, d_alpha, d_proj, zfar, znear, H, W)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    # the Python layer: prefix views of H*W-row buffers, [1,H,W] inputs as well
    pts = Sm.surface_points(d_depth[None], d_alpha[None], d_proj, zfar, znear, with_alpha=True, with_rank=True)
    assert (pts.count, pts.height, pts.width) == (want["count"], H, W)
    same_bits(pts.xyz, want["xyz"])
    same_bits(pts.index, want["index"])
    same_bits(pts.alpha, want["alpha"])
    same_bits(pts.rank, want["rank"].reshape(H, W))
    assert pts._xyz.shape == (H * W, 3) and pts.xyz.untyped_storage().data_ptr() == pts._xyz.untyped_storage().data_ptr()
    lean = Sm.surface_points(d_depth, d_alpha, d_proj, zfar, znear, with_index=False)
    assert lean.index is None and lean.alpha is None and lean.rank is None
    same_bits(lean.xyz, want["xyz"])


@pytest.mark.parametrize("H,W", [(17, 23), (B + 1, 3), (513, 512)])
def test_side_stream_reused_temp_misaligned_planes_and_other_thresholds(H, W):
    """One `temp` serves call after call on a stream that is not the default one; planes that start 4 bytes past a 16-byte boundary
    take the dword loads and give the same bits; the threshold is the caller's."""
    from texgs import surface as Sm
    depth, proj, zfar, znear, world, masks = scene(H, W)
    n = H * W
    d_proj = dev(proj)
    temp = torch.empty(Sm.entry().texgs_surface_temp_bytes(H, W) // 8, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    d_depth_off = torch.empty(n + 1, dtype=torch.float32, device=DEV)
    d_depth_off[1:] = dev(depth).reshape(-1)
    runs = []
    for name, thr in (("random", 0.5), ("runs", 0.5), ("random", 0.25), ("special", -1.0), ("random", 0.9)):
        alpha = masks[name]
        d_alpha_off = torch.empty(n + 1, dtype=torch.float32, device=DEV)
        d_alpha_off[1:] = dev(alpha).reshape(-1)
        assert d_alpha_off[1:].data_ptr() % 16 == 4
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            outs = c_call(d_depth_off[1:], d_alpha_off[1:], d_proj, zfar, znear, H, W, threshold=thr, temp=temp, stream=side)
        runs.append((outs, expected(H, W, alpha, thr), d_alpha_off))
    side.synchronize()
    for outs, want, _ in runs:
        check_c_outputs(outs, want, n)
    assert len({w["count"] for _, w, _ in runs}) > 2


def test_optional_outputs_may_be_null():
    H, W = 17, 23
    depth, proj, zfar, znear, world, masks = scene(H, W)
    want = expected(H, W, masks["random"])
    count, xyz, index, asel, rank = c_call(dev(depth), dev(masks["random"]), dev(proj), zfar, znear, H, W, outputs=())
    assert index is None and asel is None and rank is None and int(count.cpu()[0]) == want["count"]
    same_bits(xyz[:want["count"]], want["xyz"])


def test_a_nan_depth_reaches_only_its_own_row():
    from texgs import surface as Sm
    H, W = 17, 23
    depth, proj, zfar, znear, world, masks = scene(H, W)
    alpha = masks["all"]
    clean = Sm.surface_points(dev(depth), dev(alpha), dev(proj), zfar, znear).xyz.cpu().numpy()
    bad = depth.copy()
    bad[5, 7] = np.nan
    bad[9, 1] = np.inf
    got = Sm.surface_points(dev(bad), dev(alpha), dev(proj), zfar, znear)
    same_bits(got.xyz, R.world_points(bad, proj, zfar, znear))
    got = got.xyz.cpu().numpy()
    rows = [5 * W + 7, 9 * W + 1]
    assert np.isnan(got[rows[0]]).all() and not np.isfinite(got[rows[1]]).any()
    keep = np.setdiff1d(np.arange(H * W), rows)
    assert np.array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    # under the mask's complement a NaN depth is never read into a row
    alpha2 = alpha.copy()
    alpha2[5, 7] = 0.25
    alpha2[9, 1] = 0.25
    got2 = Sm.surface_points(dev(bad), dev(alpha2), dev(proj), zfar, znear)
    assert got2.count == H * W - 2 and bool(torch.isfinite(got2.xyz).all())
    same_bits(got2.xyz, clean[keep])


def test_golden_map_on_the_device_is_within_a_float32_rounding_of_the_reference_points():
    from texgs import surface as Sm
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_terms.npz"))
    got = Sm.surface_points(dev(d["d2w_depth"]), torch.ones(17, 23, device=DEV), dev(d["d2w_full_proj"]), float(d["d2w_zfar"]), float(d["d2w_znear"]))
    want = d["d2w_xyz64"].reshape(-1, 3)
    same_bits(got.xyz, R.world_points(d["d2w_depth"], d["d2w_full_proj"], float(d["d2w_zfar"]), float(d["d2w_znear"])))
    err = np.abs(got.xyz.cpu().numpy().astype(np.float64) - want)
    assert (err <= 1e-6 + 2.0 ** -24 * np.abs(want)).all(), err.max()


@pytest.mark.parametrize("H,W", [(1, 1), (17, 23), (1, B + 1), (B + 1, 3), (64, 64)])
def test_compose_equals_the_statement(H, W):
    from texgs import surface as Sm
    depth, proj, zfar, znear = R.make_depth(H, W, 1), *R.camera(H, W, 1)
    masks = R.masks(H, W, B)
    d_depth, d_proj = dev(depth), dev(proj)
    rng = np.random.default_rng(H * W)
    for name in ("none", "random", "all", "special"):
        alpha = masks[name]
        d_alpha = dev(alpha)
        pts = Sm.surface_points(d_depth, d_alpha, d_proj, zfar, znear, with_rank=True)
        values = rng.random((pts.count, 3)).astype(R.F)
        if name == "none":
            assert pts.count == 0
        rank = pts.rank.cpu().numpy()
        d_values = dev(values) if pts.count else torch.zeros(0, 3, device=DEV)
        same_bits(Sm.compose(pts, d_values, d_alpha), R.compose(values, rank, alpha))
        same_bits(Sm.compose(pts, d_values, d_alpha[None], background=dev(R.BACKGROUND)), R.compose(values, rank, alpha, R.BACKGROUND))
        same_bits(Sm.compose(pts, d_values, d_alpha, background=[float(v) for v in R.BACKGROUND]), R.compose(values, rank, alpha, R.BACKGROUND))
        with pytest.raises(ValueError, match="rows, the points are"):
            Sm.compose(pts, torch.zeros(pts.count + 1, 3, device=DEV), d_alpha)


def test_compose_is_the_reference_scatter_add():
    """uv_map_gaussian3d.py:283-286 in torch on the device, as values (the reference adds into the background term too)"""
    from texgs import surface as Sm
    H, W = 33, 65
    depth, proj, zfar, znear = R.make_depth(H, W, 2), *R.camera(H, W, 2)
    alpha = dev(R.masks(H, W, B)["random"])
    pts = Sm.surface_points(dev(depth), alpha, dev(proj), zfar, znear, with_rank=True)
    g = torch.Generator().manual_seed(4)
    rgb = torch.rand(pts.count, 3, generator=g).to(DEV)
    bg = dev(R.BACKGROUND)
    valid = alpha.reshape(-1) > 0.5
    index = torch.arange(H * W, device=DEV)[valid]
    assert torch.equal(index, pts.index)
    src = alpha.reshape(-1)[valid][:, None] * rgb
    ref = bg.reshape(1, 3).repeat(H * W, 1) * (1 - alpha).reshape(-1, 1)
    ref = ref.scatter_add(dim=0, index=index[:, None].repeat(1, 3), src=src).reshape(H, W, 3).permute(2, 0, 1)
    assert torch.equal(Sm.compose(pts, rgb, alpha, bg), ref.contiguous())


def _uv_net():
    from texgs.uvnet import UVNet
    torch.manual_seed(2)
    return UVNet(precision="fp32").to(DEV)


def test_chess_image_is_its_four_pieces():
    from texgs import cubetex, surface as Sm
    H, W = 48, 40
    depth, proj, zfar, znear = R.make_depth(H, W, 3), *R.camera(H, W, 3)
    alpha = dev(R.masks(H, W, B)["random"])
    d_depth, d_proj = dev(depth), dev(proj)
    net = _uv_net()
    emb = (torch.randn(128, generator=torch.Generator().manual_seed(1)) * 0.1).to(DEV)
    for bg in (None, dev(R.BACKGROUND)):
        got = Sm.chess_image(d_depth[None], alpha[None], d_proj, zfar, znear, net, emb, background=bg)
        pts = Sm.surface_points(d_depth, alpha, d_proj, zfar, znear, with_rank=True)
        uv, _ = net.uv_and_jacobian(pts.xyz, emb)
        rgb = cubetex.chessboard_texture(uv)
        want = Sm.compose(pts, rgb.reshape(-1, 3).contiguous(), alpha, bg)
        assert got.shape == (3, H, W) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert 0 < pts.count < H * W and bool((got[:, pts.rank >= 0].amax(0) > 0).all())
    # nothing selected: the background term everywhere, no network call
    none = torch.zeros(H, W, device=DEV)
    same_bits(Sm.chess_image(d_depth, none, d_proj, zfar, znear, None, emb, background=dev(R.BACKGROUND)),
              np.broadcast_to(R.BACKGROUND[:, None, None], (3, H, W)).copy())


def test_uv_map_loss_takes_the_given_points():
    from texgs import surface as Sm, uvmap
    from texgs.losses import depth2world
    H, W = 48, 40
    depth, proj, zfar, znear = R.make_depth(H, W, 4), *R.camera(H, W, 4)
    alpha = dev(R.masks(H, W, B)["random"])[None]
    d_depth, d_proj = dev(depth)[None], dev(proj)
    uv_net = _uv_net()
    inv_net = uvmap.InvUVNet(n_sample_points=512)
    with torch.no_grad():
        inv_net.encoding.params.uniform_(-0.3, 0.3)
    inv_net = inv_net.to(DEV)
    emb = (torch.randn(128, generator=torch.Generator().manual_seed(1)) * 0.1).to(DEV)
    pcd = torch.randn(700, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    cfg = uvmap.UVMapLossCfg(lambda_inverse=1.0, lambda_chamfer=1.0, lambda_patch_chamfer=0.0, lambda_inverse2=1.0)
    run = lambda d, a, **kw: uvmap.uv_map_loss(d, a, d_proj, znear, zfar, uv_net, inv_net, emb, pcd, cfg,
                                               generator=torch.Generator().manual_seed(9), **kw)

    def same(x, y):
        assert x[1].keys() == y[1].keys()
        return all(torch.equal(x[1][k].detach().view(torch.int32), y[1][k].detach().view(torch.int32)) for k in x[1])

    default = run(d_depth, alpha)
    # the default path's own points, handed in: the same bits
    own = depth2world(d_depth[0], d_proj, zfar, znear).reshape(-1, 3)[alpha.reshape(-1) > 0.5].contiguous()
    assert same(default, run(d_depth, alpha, world_xyz=own))
    # the stage's points differ from those in the last bits; with them the loss is computed from exactly these rows, whatever the maps say
    pts = Sm.surface_points(d_depth, alpha, d_proj, zfar, znear)
    assert pts.xyz.shape == own.shape and not torch.equal(pts.xyz, own) and float((pts.xyz - own).abs().max()) < 1e-3
    given = run(d_depth, alpha, world_xyz=pts.xyz)
    assert same(given, run(torch.full_like(d_depth, 9.0), torch.ones_like(alpha), world_xyz=pts.xyz))
    with torch.no_grad():
        uv, _ = uv_net.uvs_and_jacobian_with_grad(pts.xyz, emb)
        linv = ((pts.xyz - inv_net(uv, emb)) ** 2).sum(-1).mean()
    assert torch.equal(given[1]["Linv"].detach().view(torch.int32), linv.view(torch.int32))


def test_wait_false_returns_the_same_after_other_work_was_queued():
    from texgs import surface as Sm
    H, W = 513, 512
    depth, proj, zfar, znear, world, masks = scene(H, W)
    want = expected(H, W, masks["random"])
    d_depth, d_alpha, d_proj = dev(depth), dev(masks["random"]), dev(proj)
    pts = Sm.surface_points(d_depth, d_alpha, d_proj, zfar, znear, with_alpha=True, with_rank=True, wait=False)
    assert pts._count is None and pts.rank is not None and (pts.height, pts.width) == (H, W)        # these never wait
    other = Sm.surface_points(d_depth, dev(masks["alternate"]), d_proj, zfar, znear, wait=False)      # more work behind it, same stream
    busy = (torch.randn(512, 512, device=DEV) @ torch.randn(512, 512, device=DEV)).sum()
    assert pts._count is None and other._count is None
    same_bits(pts.xyz, want["xyz"])                     # the first access waits
    assert pts._count == want["count"] == pts.count
    same_bits(pts.index, want["index"])
    same_bits(pts.alpha, want["alpha"])
    same_bits(pts.rank, want["rank"].reshape(H, W))
    assert other.count == (H * W + 1) // 2 and bool(torch.isfinite(busy))
    same_bits(other.xyz, world[::2])
