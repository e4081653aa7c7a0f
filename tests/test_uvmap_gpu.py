"""-m gpu: the UV-map stage's HIP kernels (csrc/uvmap.hip) and texgs.uvmap against float64 statements: the hash-grid encoding
(tests/hashgrid_ref.py) forward, d theta and d x; InvUVNet against a plain float64 copy; chamfer against brute force; uv_map_loss
on a small synthetic scene against an all-float64 recomputation.

Bars.  fp32 unit roundoff u = 2^-24 ~ 6e-8.  The kernel rounds pos = scale x + 0.5 once (fmaf): for pos < 256 (the finest shipped
level has scale 212.2) that is at most half an ulp of 256, 2^-17 ~ 7.6e-6 of a cell, so each fraction f_d is off by at most E_F =
7.6e-6 (+ a few u).  Every trilinear weight moves by at most sum_d |dw/df_d| E_F <= 3 E_F, and sum_c |dw_c/df_d| = 2, so one level's
value moves by at most 3 * 2 * E_F * max|theta| (+ 8 fp32 fmas).  Those are the encoding bars; the others are derived next to them."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashgrid_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
E_F = 2.0 ** -17 + 8 * 2.0 ** -24
DEV = "cuda:0"


def _params(g, n=131072, amp=1.0):
    return ((torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * amp).float()


def _points(g, N):
    """random points, points on cell faces of level 0 and level 7, every x in {0, 1}^3, and a few just outside [0, 1]"""
    lv, _ = R.levels(**R.SHIPPED)
    rnd = torch.rand(N, 3, generator=g, dtype=torch.float64)
    face0 = ((torch.randint(0, 16, (64, 3), generator=g).double() - 0.5) / lv[0][0]).clamp(0, 1)
    face7 = ((torch.randint(0, 213, (64, 3), generator=g).double() - 0.5) / lv[7][0]).clamp(0, 1)
    corners = torch.tensor([[(c >> k) & 1 for k in range(3)] for c in range(8)], dtype=torch.float64)
    out = torch.tensor([[-0.01, 0.5, 1.01], [1.003, -0.002, 0.25]], dtype=torch.float64)
    return torch.cat([rnd, face0, face7, corners, out]).float()


@pytest.mark.parametrize("N", [1237, 0])
def test_encoding_forward(lib_built, N):
    from texgs import uvmap
    g = torch.Generator().manual_seed(11 + N)
    x = _points(g, N) if N else torch.zeros(0, 3)
    params = _params(g)
    enc = uvmap.hashgrid_encode(x.to(DEV), params.to(DEV))
    torch.cuda.synchronize()
    assert enc.shape == (x.shape[0], 32)
    ref = R.encode(x.double(), params.double())
    bar = 3 * 2 * E_F * 1.0 + 8 * 2 * 2.0 ** -24                    # max|theta| = 1
    err = (enc.cpu().double() - ref).abs().max() if x.shape[0] else torch.tensor(0.0)
    assert float(err) <= bar, (float(err), bar)


def _touch_sums(x, de):
    """per table entry: the sum over the (point, corner) terms that add into it of |d_enc|, and the number of those terms
    (float64, from the statement's corners)"""
    lv, n = R.levels(**R.SHIPPED)
    out = torch.zeros(n // 4, 4, dtype=torch.float64)
    cnt = torch.zeros(n // 4, dtype=torch.int64)
    x = x.double()
    for l, (s, res, size, off, hashed) in enumerate(lv):
        gi = torch.floor(x * s + 0.5).long() & R.M32
        for c in range(8):
            idx = R.corner_index(gi[:, 0] + (c & 1), gi[:, 1] + ((c >> 1) & 1), gi[:, 2] + (c >> 2), res, size, hashed)
            out.index_add_(0, off + idx, de[:, 4 * l:4 * l + 4].abs().double())
            cnt.index_add_(0, off + idx, torch.ones_like(idx))
    return out.reshape(-1), cnt.repeat_interleave(4)


@pytest.mark.parametrize("N", [3001, 40000])
def test_encoding_backward(lib_built, N):
    from texgs import uvmap
    g = torch.Generator().manual_seed(N)
    x = _points(g, N)
    params = _params(g)
    de = torch.randn(x.shape[0], 32, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    pd = params.to(DEV).requires_grad_(True)
    uvmap.hashgrid_encode(xd, pd).backward(de.to(DEV))
    x64 = x.double().requires_grad_(True)
    p64 = params.double().requires_grad_(True)
    (R.encode(x64, p64) * de.double()).sum().backward()

    # d theta: every term w_c d_enc is off by at most 3 E_F |d_enc| (weights) + u |term|; an fp32 sum of k terms in any order (LDS
    # atomics, then the global flush) is off by at most (k - 1) u sum|terms|.  With T = sum |d_enc| over an entry's terms (>= sum
    # |terms|, since w <= 1) and k_max the largest term count of any entry (level 0 at N = 40000: ~40000 * 8 / 4096 ~ 80 on average),
    # the bar is (3 E_F + (k_max + 1) u) T -- plus one term's worth where a point within rounding of a face lands in the
    # neighbouring cell (its weight there is <= 3 E_F).
    got = pd.grad.cpu().double()
    T, count = _touch_sums(x, de)
    k_max = int(count.max())
    bar = (3 * E_F + (k_max + 1) * 2.0 ** -24) * T + 3 * E_F * float(de.abs().max())
    assert bool(((got - p64.grad).abs() <= bar).all()), float(((got - p64.grad).abs() - bar).max())
    rel = float((got - p64.grad).norm() / p64.grad.norm())
    assert rel < 1e-5, rel

    # d x: the gradient jumps across a cell face; points within rounding (2 E_F cells) of a face at any level are excluded and counted.
    # Elsewhere: d enc / d x_d = scale_l sum_c (+-) prod_{e != d} w_e theta -- the two other weights are off by <= E_F each, so one
    # level's share is off by <= scale_l * 8 corners * 2 E_F * sum_j |d_enc_j| max|theta|, plus ~64 u of the same for rounding.
    far = R.face_distance(x) > 2 * E_F
    assert int((~far).sum()) <= 64 + 64 + N // 200, int((~far).sum())       # the constructed face points + chance hits (~1e-3 per point)
    lv, _ = R.levels(**R.SHIPPED)
    bound = sum(s * (16 * E_F + 64 * 2.0 ** -24) * de[:, 4 * l:4 * l + 4].abs().sum(1).double() for l, (s, *_r) in enumerate(lv))
    gx = xd.grad.cpu().double()
    dx_err = (gx - x64.grad).abs().max(dim=1).values
    assert bool((dx_err[far] <= bound[far]).all()), float((dx_err[far] - bound[far]).max())


def test_encoding_backward_empty(lib_built):
    from texgs import uvmap
    xd = torch.zeros(0, 3, device=DEV, requires_grad=True)
    pd = torch.zeros(131072, device=DEV, requires_grad=True)
    uvmap.hashgrid_encode(xd, pd).sum().backward()
    torch.cuda.synchronize()
    assert xd.grad.shape == (0, 3) and float(pd.grad.abs().sum()) == 0.0


class _PlainInv(torch.nn.Module):
    """float64 plain-torch copy of InvUVNet: the statement's encoding + nn.Linear layers, autograd everywhere"""

    def __init__(self, net):
        super().__init__()
        self.table = torch.nn.Parameter(net.encoding.params.detach().cpu().double().clone())
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(w.detach().cpu().double().clone()) for w in net._weights()])
        self.scale = None if net.xyz_scale is None else net.xyz_scale.cpu().double()
        self.offset = None if net.xyz_offset is None else net.xyz_offset.cpu().double()

    def forward(self, uv, emb, uv32=None):
        """uv32: the fp32 inputs the GPU net saw -- the float64 encoding then takes the cells fp32 takes (see hashgrid_ref.encode)"""
        W1, W2, W3, W4, W5 = self.ws
        e = R.encode(uv / 2 + 0.5, self.table, cells=None if uv32 is None else uv32.float().cpu() / 2 + 0.5)
        h = torch.relu(torch.relu(e @ W1.t()) @ W2.t() + emb)
        o = torch.relu(torch.relu(h @ W3.t()) @ W4.t()) @ W5.t()
        return o if self.scale is None else o * self.scale + self.offset


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm() / b.detach().double().cpu().norm().clamp_min(1e-30))


@pytest.mark.parametrize("N", [3000, 20001])            # 20001 >= 8 x 2048: the chunked weight gradients (uvnet._tn)
def test_inv_uv_net_against_plain_torch(lib_built, N):
    from texgs import uvmap
    torch.manual_seed(5)
    net = uvmap.InvUVNet(xyz_offset=[0.1, -0.2, 0.05], xyz_scale=[1.5, 0.8, 1.2])
    with torch.no_grad():
        net.encoding.params.uniform_(-0.5, 0.5)
    plain = _PlainInv(net)
    net = net.to(DEV)
    g = torch.Generator().manual_seed(N)
    uv = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    emb = torch.randn(128, generator=g) * 0.1
    w = torch.randn(N, 3, generator=g)
    uvd, embd = uv.to(DEV).requires_grad_(True), emb.to(DEV).requires_grad_(True)
    out = net(uvd, embd)
    (out * w.to(DEV)).sum().backward()
    uv64, emb64 = uv.double().requires_grad_(True), emb.double().requires_grad_(True)
    ref = plain(uv64, emb64, uv32=uv)
    (ref * w.double()).sum().backward()
    # values: the encoding within 6 E_F * 0.5 absolute (see the module docstring), then five fp32 GEMMs of K <= 128 (~ K u relative
    # each): 1e-4 relative L2 covers both with margin.  Gradients: the same per-layer rounding, plus ReLU pre-activations within
    # rounding of 0 that flip between fp32 and float64.  A flip at one unit of one point drops or adds that unit's share of the
    # point's gradient (~1/sqrt(128) of it); at ~5e-4 flips per point (512 units, pre-activations within ~1e-6 of 0) the relative
    # L2 of a sum over N points of random sign is ~sqrt(5e-4 / 128) ~ 2e-3: bar 5e-3.  (The encoding's cells are fp32's, above.)
    assert _rel(out, ref) < 1e-4, _rel(out, ref)
    assert _rel(uvd.grad, uv64.grad) < 5e-3, _rel(uvd.grad, uv64.grad)
    assert _rel(embd.grad, emb64.grad) < 5e-3
    assert _rel(net.encoding.params.grad, plain.table.grad) < 5e-3
    for k, (wg, wr) in enumerate(zip(net._weights(), plain.ws)):
        assert _rel(wg.grad, wr.grad) < 5e-3, (k, _rel(wg.grad, wr.grad))


def _brute(a, b):
    """float64 nearest neighbours: (d2, idx lowest on ties, gap to the second nearest)"""
    D = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    d2, idx = D.min(dim=1)
    D2 = D.clone()
    D2[torch.arange(a.shape[0]), idx] = float("inf")
    return d2, idx, D2.min(dim=1).values - d2


@pytest.mark.parametrize("single", [False, True])
def test_chamfer_against_brute_force(lib_built, single):
    from texgs import uvmap
    g = torch.Generator().manual_seed(3)
    P, Q = 2048, 16384
    x = torch.randn(P, 3, generator=g)
    y = torch.randn(Q, 3, generator=g)
    y[1000:1100] = y[10:110]                    # exact duplicates: the lower index must win
    x[:50] = y[200:250]                         # zero distances
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss, none = uvmap.chamfer_distance(xd[None], yd[None], single_directional=single)
    assert none is None
    loss.backward()
    d2x, ix = uvmap.nearest_neighbours(x.to(DEV), y.to(DEV))
    d2y, iy = uvmap.nearest_neighbours(y.to(DEV), x.to(DEV))
    x64, y64 = x.double(), y.double()
    rx, rix, gapx = _brute(x64, y64)
    ry, riy, gapy = _brute(y64, x64)
    # a distance is a sum of three fp32 squares of fp32 differences: relative error <= ~5u; two candidates whose float64 gap is
    # below 1e-6 * d2 (+ 1e-30) may legitimately swap order in fp32.  Exact ties (duplicates) are resolved identically.
    for got_i, ref_i, gap, ref_d in ((ix.cpu(), rix, gapx, rx), (iy.cpu(), riy, gapy, ry)):
        clear = gap > 1e-6 * ref_d + 1e-30
        assert torch.equal(got_i[clear], ref_i[clear])
        assert torch.equal(got_i[gap == 0], ref_i[gap == 0])            # exact ties: lowest index
    assert float((d2x.cpu().double() - rx).abs().max()) <= float(5 * 2.0 ** -24 * rx.max() + 1e-12)
    # loss and gradients: float64 autograd with the kernel's choice where the two sets are within rounding (same minimum value)
    ixc, iyc = ix.cpu(), iy.cpu()
    xa, ya = x64.clone().requires_grad_(True), y64.clone().requires_grad_(True)
    ref = ((xa - ya[ixc]) ** 2).sum(-1).mean()
    if not single:
        ref = ref + ((ya - xa[iyc]) ** 2).sum(-1).mean()
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)           # a mean of values with <= 5u relative error
    # per-entry gradient terms 2 (x - y) / P carry the fp32 subtraction's half-ulp: 1e-5 relative L2
    assert _rel(xd.grad, xa.grad) < 1e-5
    assert _rel(yd.grad, ya.grad) < 1e-5


def test_uv_map_loss_against_float64(lib_built):

    from texgs import synth, uvmap
    from texgs.rasterizer import GaussianRasterizationSettings
    from texgs.uvnet import UVNet
    scene = synth.make_scene(3000, 4, seed=7, scale_mean=0.03)
    cam = synth.fibonacci_cameras(6, 128, 96)[2]
    st = GaussianRasterizationSettings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
                                       tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.zeros(3, device=DEV), scale_modifier=1.0,
                                       viewmatrix=cam.world_view_transform.to(DEV), projmatrix=cam.full_proj_transform.to(DEV),
                                       sh_degree=0, campos=cam.camera_center.to(DEV), prefiltered=False, debug=False)
    f = lambda t: t.float().to(DEV).contiguous()
    depth, alpha = uvmap.render_depth_alpha(st, f(scene.means3D), f(scene.opacities), f(scene.scales), f(scene.rotations))
    n_valid = int((alpha > 0.5).sum())
    assert n_valid > 1000, n_valid
    torch.manual_seed(2)
    uv_net = UVNet(precision="fp32")
    inv_net = uvmap.InvUVNet()
    with torch.no_grad():
        inv_net.encoding.params.uniform_(-0.3, 0.3)
    geo_emb = torch.nn.Embedding(1, 128)
    with torch.no_grad():
        geo_emb.weight.mul_(0.1)
    pcd = scene.means3D[torch.randperm(3000, generator=torch.Generator().manual_seed(1))[:1500]].float()
    uv64 = UVNet(precision="fp32").double()
    uv64.load_state_dict(uv_net.state_dict())
    inv64 = _PlainInv(inv_net)
    emb64 = torch.nn.Parameter(geo_emb.weight.detach()[0].double().clone())
    uv_net, inv_net, geo_emb = uv_net.to(DEV), inv_net.to(DEV), geo_emb.to(DEV)
    cfg = uvmap.UVMapLossCfg(lambda_inverse=1.0, lambda_chamfer=1.0, lambda_patch_chamfer=0.5, lambda_inverse2=1.0)
    znear, zfar = 0.01, 100.0
    loss, stats = uvmap.uv_map_loss(depth, alpha, f(cam.full_proj_transform), znear, zfar, uv_net, inv_net, geo_emb, pcd.to(DEV), cfg,
                                    generator=torch.Generator().manual_seed(9))
    loss.backward()

    # float64 recomputation, same samples (the same CPU generator sequence), brute-force chamfer
    gen = torch.Generator().manual_seed(9)
    # depth2world checked independently of its own formula first: with a float64 projection, the pixel-centre rays scaled to the
    # rendered view depth and moved to world space by the inverse view matrix alone (x_view = ndc_x d tan(fovx/2), ...)
    d64 = depth[0].cpu().double()
    H, W = d64.shape
    ndc_y, ndc_x = torch.meshgrid((torch.arange(H, dtype=torch.float64) * 2 + 1) / H - 1,
                                  (torch.arange(W, dtype=torch.float64) * 2 + 1) / W - 1, indexing="ij")
    view = torch.stack([ndc_x * d64 * math.tan(cam.FoVx / 2), ndc_y * d64 * math.tan(cam.FoVy / 2), d64, torch.ones_like(d64)], -1)
    geo = (view.reshape(-1, 4) @ torch.linalg.inv(cam.world_view_transform.double()))[:, :3]
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    Pc = torch.zeros(4, 4, dtype=torch.float64)
    Pc[0, 0], Pc[1, 1], Pc[3, 2] = 1 / tx, 1 / ty, 1.0
    Pc[2, 2], Pc[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    P64 = cam.world_view_transform.double() @ Pc.t()
    # (depth2world inverts P, whose z and w columns are parallel to 1 part in zfar / znear = 1e4: the float64 inverse is good to
    # ~1e-8 here; 1e-6 is far below the ~1e-5 shift the float32-rounded matrix gives both sides below)
    assert torch.allclose(uvmap.depth2world(d64, P64, zfar, znear).reshape(-1, 3), geo, rtol=0, atol=1e-6)
    # the recomputation then uses the matrix the fp32 path was given (float32-rounded: the reference's formula does not divide by
    # the homogeneous coordinate, so that rounding moves points by ~1e-5 -- the same for both sides)
    world = uvmap.depth2world(d64, cam.full_proj_transform.double(), zfar, znear).reshape(-1, 3)
    wx = world[(alpha.reshape(-1) > 0.5).cpu()]
    uv = uv64(wx, emb64)
    with torch.no_grad():          # what the fp32 path fed the inverse net (same kernels, same inputs: the same values)
        wx32 = uvmap.depth2world(depth[0], f(cam.full_proj_transform), zfar, znear).reshape(-1, 3)[alpha.reshape(-1) > 0.5].contiguous()
        uv32 = uv_net.uv_and_jacobian(wx32, geo_emb.weight[0])[0]
        s_uv32 = inv_net.sample(device=DEV, generator=gen)
    Linv = ((wx - inv64(uv, emb64, uv32=uv32)) ** 2).sum(-1).mean()
    s_uv = s_uv32.double().cpu()
    s_xyz = inv64(s_uv, emb64, uv32=s_uv32)
    p64 = pcd.double()
    _, ia, _ = _brute(s_xyz.detach(), p64)
    _, ib, _ = _brute(p64, s_xyz.detach())
    Lch = ((s_xyz - p64[ia]) ** 2).sum(-1).mean() + ((p64 - s_xyz[ib]) ** 2).sum(-1).mean()
    Lpatch = ((s_xyz - p64[ia]) ** 2).sum(-1).mean()             # the uniform samples are reused (the reference's sharing)
    Linv2 = ((uv64(s_xyz, emb64) - s_uv) ** 2).sum(-1).mean()
    total = Linv + Lch + 0.5 * Lpatch + Linv2
    total.backward()
    # every term is a mean over >= 1000 points of values from fp32 networks whose outputs are ~1e-5 relative (K <= 128 GEMMs, the
    # encoding bar above) and fp32 depth2world (~1e-6): 1e-4 relative per term.  Gradients: the same, plus ReLU pre-activations
    # within rounding of 0 that flip, in both nets (see test_inv_uv_net_against_plain_torch): 1e-2 relative L2.
    for name, ref in (("Linv", Linv), ("Lchamfer", Lch), ("Lpatch_chamfer", Lpatch), ("Linv2", Linv2), ("total_loss", total)):
        assert abs(float(stats[name]) - float(ref)) <= 1e-4 * abs(float(ref)), (name, float(stats[name]), float(ref))
    for (n, p), (n2, q) in zip(uv_net.named_parameters(), uv64.named_parameters()):
        assert _rel(p.grad, q.grad) < 1e-2, (n, _rel(p.grad, q.grad))
    assert _rel(inv_net.encoding.params.grad, inv64.table.grad) < 1e-2
    for k, (w, q) in enumerate(zip(inv_net._weights(), inv64.ws)):
        assert _rel(w.grad, q.grad) < 1e-2, (k, _rel(w.grad, q.grad))
    assert _rel(geo_emb.weight.grad[0], emb64.grad) < 1e-2
