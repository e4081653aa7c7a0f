"""-m gpu: the UV-map stage's HIP kernels (csrc/uvmap.hip) and texgs.uvmap against float64 statements: the hash-grid encoding
(tests/hashgrid_ref.py) forward, d theta and d x; InvUVNet against a plain float64 copy; chamfer against brute force; uv_map_loss
on a small synthetic scene against an all-float64 recomputation.  The second half repeats the encoding checks on the grids of
hashgrid_ref.GRIDS (both backward kernels, dense levels of any size, L = 1 ... 16), calls the backward ABI in each of its gradient
modes, and takes the chamfer search to partial blocks, partial splits, ties and non-finite rows.

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
    T, count = R.touch_sums(x, de)
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

    def __init__(self, net, grid=None):
        super().__init__()
        self.grid = dict(grid or {})
        self.table = torch.nn.Parameter(net.encoding.params.detach().cpu().double().clone())
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(w.detach().cpu().double().clone()) for w in net._weights()])
        self.scale = None if net.xyz_scale is None else net.xyz_scale.cpu().double()
        self.offset = None if net.xyz_offset is None else net.xyz_offset.cpu().double()

    def forward(self, uv, emb, uv32=None):
        """uv32: the fp32 inputs the GPU net saw -- the float64 encoding then takes the cells fp32 takes (see hashgrid_ref.encode)"""
        W1, W2, W3, W4, W5 = self.ws
        e = R.encode(uv / 2 + 0.5, self.table, cells=None if uv32 is None else uv32.float().cpu() / 2 + 0.5, **self.grid)
        h = torch.relu(torch.relu(e @ W1.t()) @ W2.t() + emb)
        o = torch.relu(torch.relu(h @ W3.t()) @ W4.t()) @ W5.t()
        return o if self.scale is None else o * self.scale + self.offset

    @torch.no_grad()
    def kink_distance(self, uv, emb, uv32=None):
        """per point: the smallest |pre-activation| of any ReLU unit, relative to the largest |pre-activation| of its layer"""
        W1, W2, W3, W4, _ = self.ws
        z = R.encode(uv / 2 + 0.5, self.table, cells=None if uv32 is None else uv32.float().cpu() / 2 + 0.5, **self.grid) @ W1.t()
        best = torch.full((uv.shape[0],), float("inf"), dtype=torch.float64)
        for W, add in ((W2, emb), (W3, 0.0), (W4, 0.0), (None, 0.0)):
            best = torch.minimum(best, z.abs().min(dim=1).values / z.abs().max())
            if W is not None:
                z = torch.relu(z) @ W.t() + add
        return best


def _rel(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm() / b.detach().double().cpu().norm().clamp_min(1e-30))


def _inv_uv_net_against_plain_torch(N, grid=None, kink_margin=None):
    """kink_margin: points with a ReLU pre-activation (float64) within that fraction of its layer's largest one of zero get the
    loss weight 0 on both sides, and are counted.  fp32 and float64 can switch such a unit differently, and one such flip moves a
    weight gradient's relative L2 by several 1e-3 at N = 3000: measured 5.05e-3 for one flipped unit of the last hidden layer on
    the mixed grid, in the MI355X run and in a plain fp32 torch twin on the CPU alike -- so with no kernel of this project
    involved; the estimate in the comment below is too low for a single unlucky flip.  An fp32 pre-activation is within ~1e-5 of
    the float64 one (the encoding bar 6 E_F * 0.5 ~ 1e-5 absolute, then GEMMs of K <= 128 at ~1e-6 relative), so a margin of 1e-4
    of the layer's largest pre-activation leaves a factor of 10: a unit outside it does not flip.  Every point still runs
    through every kernel; only the loss weight of the excluded ones is zero."""
    from texgs import uvmap
    torch.manual_seed(5)
    net = uvmap.InvUVNet(xyz_offset=[0.1, -0.2, 0.05], xyz_scale=[1.5, 0.8, 1.2], grid=grid)
    with torch.no_grad():
        net.encoding.params.uniform_(-0.5, 0.5)
    plain = _PlainInv(net, grid)
    net = net.to(DEV)
    g = torch.Generator().manual_seed(N)
    uv = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    emb = torch.randn(128, generator=g) * 0.1
    w = torch.randn(N, 3, generator=g)
    if kink_margin is not None:
        near = plain.kink_distance(uv.double(), emb.double(), uv32=uv) < kink_margin
        # 512 units per point, pre-activations spread like a Gaussian whose 4 sigma is the layer's maximum: density 1.6 / max at
        # zero, so a unit is inside the margin with probability 2 * 1.6 * kink_margin, a point with 512 times that: 16 % at 1e-4
        assert 0 < int(near.sum()) <= N // 4, int(near.sum())
        w[near] = 0.0
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


@pytest.mark.parametrize("N", [3000, 20001])            # 20001 >= 8 x 2048: the chunked weight gradients (uvnet._tn)
def test_inv_uv_net_against_plain_torch(lib_built, N):
    _inv_uv_net_against_plain_torch(N)


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


# ---- off the shipped grid ---------------------------------------------------------------------------------------------------
# The shipped grid has 4096 rows at every level: each level sits exactly on the LDS-slab limit of the backward (size * 16 B <= 64 KiB),
# so nothing above reaches the global-atomic kernel with a parameter gradient, a call that uses both launches, a dense level that
# is no power of two, or L != 8.  hashgrid_ref.GRIDS does.  The bars are the ones above with E_F = R.rounding_bar(1.15, grid): the
# points now reach [-0.15, 1.15]^3 (x is not clamped; a negative floor wraps to uint32 as the statement's does).
U = 2.0 ** -24
X_MAX = 1.15
N_SPECIAL = 64 + 64 + 8 + 2 + 64
GRID_CASES = [("mixed", N) for N in (1, 511, 512, 513, 3001)] \
    + [(name, N) for name in ("small_dense", "L16", "L1", "tiny_hash") for N in (3001, 20000)]
_cases = {}


def _grid_points(g, N, grid):
    """N points: random ones in [0, 1]^3, then (when N leaves room) 64 on cell faces of the coarsest level, 64 on faces of the finest,
    every x in {0, 1}^3, two just outside [0, 1] and 64 uniform in [-0.15, 1.15]^3"""
    lv, _ = R.levels(**dict(R.SHIPPED, **grid))
    rnd = torch.rand(N - N_SPECIAL if N > N_SPECIAL else N, 3, generator=g, dtype=torch.float64)
    faces = [((torch.randint(0, res, (64, 3), generator=g).double() - 0.5) / s).clamp(0, 1) for s, res, *_ in (lv[0], lv[-1])]
    corners = torch.tensor([[(c >> k) & 1 for k in range(3)] for c in range(8)], dtype=torch.float64)
    out = torch.tensor([[-0.01, 0.5, 1.01], [1.003, -0.002, 0.25]], dtype=torch.float64)
    wide = torch.rand(64, 3, generator=g, dtype=torch.float64) * (2 * X_MAX - 1) + (1 - X_MAX)
    return torch.cat([rnd] + faces + [corners, out, wide])[:N].float()


def _grid_case(name, N):
    """inputs and the float64 statement's results for one (grid, N): computed once, shared, never written to"""
    if (name, N) not in _cases:
        grid = R.GRIDS[name]
        lv, n = R.levels(**dict(R.SHIPPED, **grid))
        g = torch.Generator().manual_seed(100 * len(lv) + N)
        x = _grid_points(g, N, grid)
        params = _params(g, n)
        de = torch.randn(N, 4 * len(lv), generator=g)
        x64 = x.double().requires_grad_(True)
        p64 = params.double().requires_grad_(True)
        ref = R.encode(x64, p64, **grid)
        (ref * de.double()).sum().backward()
        T, count = R.touch_sums(x, de, **grid)
        E = R.rounding_bar(X_MAX, **grid)
        # d theta per entry and d x per point: the bars derived in test_encoding_backward
        p_bar = (3 * E + (int(count.max()) + 1) * U) * T + 3 * E * float(de.abs().max())
        x_bar = sum(s * (16 * E + 64 * U) * de[:, 4 * l:4 * l + 4].abs().sum(1).double() for l, (s, *_r) in enumerate(lv))
        _cases[name, N] = dict(grid=grid, L=len(lv), x=x, params=params, de=de, ref=ref.detach(), gx=x64.grad, gp=p64.grad, E=E,
                               k_max=int(count.max()), p_bar=p_bar, x_bar=x_bar, far=R.face_distance(x, **grid) > 2 * E)
    return _cases[name, N]


def _report(label, **kw):
    import helpers
    helpers.report("uvmap_grids_" + label, **kw)


def _assert_dx(c, gx, what):
    far = c["far"]
    err = (gx.cpu().double() - c["gx"]).abs().max(dim=1).values
    assert bool((err[far] <= c["x_bar"][far]).all()), (what, float((err[far] - c["x_bar"][far]).max()))
    return float((err[far] / c["x_bar"][far]).max()) if bool(far.any()) else 0.0


def _assert_dtheta(c, got, what, extra=0.0, ref=None):
    ref = c["gp"] if ref is None else ref
    err = (got.cpu().double() - ref).abs()
    assert bool((err <= c["p_bar"] + extra).all()), (what, float((err - c["p_bar"] - extra).max()))
    return float((err / (c["p_bar"] + extra)).max())


@pytest.mark.parametrize("name,N", GRID_CASES)
def test_grid_encoding_forward(lib_built, name, N):
    """enc[i, 4 l + j] on every grid: within 6 E_F max|theta| + 16 u of the statement (max|theta| = 1), bit-equal over two runs"""
    from texgs import uvmap
    c = _grid_case(name, N)
    xd, pd = c["x"].to(DEV), c["params"].to(DEV)
    enc = uvmap.hashgrid_encode(xd, pd, grid=c["grid"])
    again = uvmap.hashgrid_encode(xd, pd, grid=c["grid"])
    torch.cuda.synchronize()
    assert enc.shape == (N, 4 * c["L"])
    bar = 6 * c["E"] * 1.0 + 16 * U
    err = (enc.cpu().double() - c["ref"]).abs()
    _report("forward", grid=name, N=N, max_err=float(err.max()), bar=bar, worst_level=int(err.max(dim=0).values.argmax()) // 4)
    assert float(err.max()) <= bar, (float(err.max()), bar)
    assert torch.equal(enc, again)


@pytest.mark.parametrize("name,N", GRID_CASES)
def test_grid_encoding_backward(lib_built, name, N):
    """d theta per entry within (3 E_F + (k_max + 1) u) T + 3 E_F max|d_enc| -- a bar that holds for any summation order, so for the
    LDS slabs and for the global atomics alike -- and d x within its bar away from cell faces, bit-equal over two runs (its level
    sum has a fixed order).  No global relative bar here: on tiny_hash an entry sums thousands of terms of either sign and the
    per-entry bar is the condition; the relative L2 error is reported."""
    from texgs import uvmap
    c = _grid_case(name, N)
    grads = []
    for _ in range(2):
        xd = c["x"].to(DEV).requires_grad_(True)
        pd = c["params"].to(DEV).requires_grad_(True)
        uvmap.hashgrid_encode(xd, pd, grid=c["grid"]).backward(c["de"].to(DEV))
        grads.append((xd.grad, pd.grad))
    (gx, gp), (gx2, _gp2) = grads
    assert gp.shape == c["params"].shape and gx.shape == (N, 3)
    near = int((~c["far"]).sum())
    assert near <= (128 if N > N_SPECIAL else 0) + N // 200, near         # the constructed face points + chance hits
    p_frac = _assert_dtheta(c, gp, "d theta")
    x_frac = _assert_dx(c, gx, "d x")
    rel = float((gp.cpu().double() - c["gp"]).norm() / c["gp"].norm())
    _report("backward", grid=name, N=N, dtheta_err_over_bar=p_frac, dtheta_max_err=float((gp.cpu().double() - c["gp"]).abs().max()),
            dtheta_rel_l2=rel, k_max=c["k_max"], dx_err_over_bar=x_frac,
            dx_max_err=float((gx.cpu().double() - c["gx"]).abs().max(dim=1).values[c["far"]].max()) if bool(c["far"].any()) else 0.0,
            near_face_points=near)
    assert torch.equal(gx, gx2)


def _hg_backward_raw(c, d_params, d_x, temp=None):
    """texgs_hashgrid_backward through ctypes, the way _HashGrid.backward calls it; d_params / d_x may be None (NULL)"""
    import ctypes as C
    from texgs import _lib, uvmap
    lib = _lib.load()
    st = uvmap._grid_struct(dict(uvmap.SHIPPED_GRID, **c["grid"]))
    N = c["x"].shape[0]
    xd, pd, ded = c["x"].to(DEV), c["params"].to(DEV), c["de"].to(DEV)
    if temp is None:
        temp = torch.empty(max(1, lib.texgs_hashgrid_backward_temp_bytes(C.byref(st), N)) if d_x is not None else 1, dtype=torch.uint8,
                           device=DEV)
    p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    rc = lib.texgs_hashgrid_backward(C.byref(st), p(pd), p(xd), p(ded), N, p(d_params), p(d_x), p(temp),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, (xd, pd, ded)


def test_grid_backward_abi_modes(lib_built):
    """The ABI: d_params is accumulated into, d_x is overwritten, either may be NULL (mixed grid: both launches; with a NULL d_params
    every level takes the kernel without a slab)."""
    c = _grid_case("mixed", 3001)
    N = 3001
    # both gradients, from zero: the reference point for the other modes
    d_p0 = torch.zeros_like(c["params"], device=DEV)
    d_x0 = torch.empty(N, 3, device=DEV)
    rc, _ = _hg_backward_raw(c, d_p0, d_x0)
    assert rc == 0
    _assert_dtheta(c, d_p0, "both: d theta")
    _assert_dx(c, d_x0, "both: d x")

    # accumulate into a pre-filled d_params, d_x = NULL.  The gradient's own error is within the d theta bar; adding it to the
    # pre-fill rounds the sum once more: u |prefill| (the |gradient| part of that rounding is inside (k_max + 1) u T).
    g = torch.Generator().manual_seed(77)
    pre = _params(g, c["params"].numel())
    d_p = pre.to(DEV)
    rc, _ = _hg_backward_raw(c, d_p, None)
    assert rc == 0
    frac1 = _assert_dtheta(c, d_p, "accumulate", extra=U * pre.double().abs(), ref=pre.double() + c["gp"])
    # a second call adds the gradient again, with its own error: twice the bar
    rc, _ = _hg_backward_raw(c, d_p, None)
    assert rc == 0
    err2 = (d_p.cpu().double() - (pre.double() + 2 * c["gp"])).abs()
    bar2 = 2 * (c["p_bar"] + U * pre.double().abs())
    assert bool((err2 <= bar2).all()), float((err2 - bar2).max())

    # d_x only: d_params = NULL, every element of a NaN-filled d_x is overwritten, bit-equal to the both-gradients call
    d_x = torch.full((N, 3), float("nan"), device=DEV)
    rc, _ = _hg_backward_raw(c, None, d_x)
    assert rc == 0
    assert not bool(torch.isnan(d_x).any())
    _assert_dx(c, d_x, "d_x only")
    assert torch.equal(d_x, d_x0)
    _report("abi_modes", grid="mixed", N=N, accumulate_err_over_bar=frac1, twice_err_over_bar=float((err2 / bar2).max()))


def test_grid_backward_neither_gradient(lib_built):
    """Both gradient pointers NULL: returns 0 before any launch -- no temp is needed (a zero-size one is passed as NULL) and the
    inputs are left as they were."""
    c = _grid_case("mixed", 3001)
    rc, (xd, pd, ded) = _hg_backward_raw(c, None, None, temp=torch.empty(0, dtype=torch.uint8, device=DEV))
    assert rc == 0
    assert torch.equal(xd.cpu(), c["x"]) and torch.equal(pd.cpu(), c["params"]) and torch.equal(ded.cpu(), c["de"])


def test_grid_backward_one_gradient_through_autograd(lib_built):
    """hashgrid_encode with only x or only the table requiring a gradient (the first passes d_params = NULL) against the
    both-gradients call: d x bit for bit, d theta within its bar."""
    from texgs import uvmap
    c = _grid_case("mixed", 3001)

    def run(need_x, need_p):
        xd = c["x"].to(DEV).requires_grad_(need_x)
        pd = c["params"].to(DEV).requires_grad_(need_p)
        uvmap.hashgrid_encode(xd, pd, grid=c["grid"]).backward(c["de"].to(DEV))
        return xd.grad, pd.grad
    gx_both, gp_both = run(True, True)
    gx_only, none_p = run(True, False)
    none_x, gp_only = run(False, True)
    assert none_p is None and none_x is None
    assert torch.equal(gx_only, gx_both)
    _assert_dx(c, gx_only, "x only")
    _assert_dtheta(c, gp_only, "params only")
    _assert_dtheta(c, gp_both, "both")


def test_inv_uv_net_off_the_shipped_grid(lib_built):
    """InvUVNet(grid=mixed): a 20-wide encoding into the MLP, the table gradient through both backward kernels.  Same bars as on the
    shipped grid; points within 1e-4 of a ReLU kink carry no loss weight (see _inv_uv_net_against_plain_torch)."""
    _inv_uv_net_against_plain_torch(3000, R.GRIDS["mixed"], kink_margin=1e-4)


# ---- chamfer nearest neighbours at the kernel's edges: a 256-lane block of queries, splits of 512 reference points ----------------
def _nn_check(a, b, label):
    """nearest_neighbours(a, b) against the float64 brute force by the rules of test_chamfer_against_brute_force"""
    from texgs import uvmap
    d2, idx = uvmap.nearest_neighbours(a.to(DEV), b.to(DEV))
    assert d2.shape == idx.shape == (a.shape[0],) and d2.dtype == torch.float32 and idx.dtype == torch.int64
    rd, ri, gap = _brute(a.double(), b.double())
    clear = gap > 1e-6 * rd + 1e-30
    assert torch.equal(idx.cpu()[clear], ri[clear])
    assert torch.equal(idx.cpu()[gap == 0], ri[gap == 0])                # exact ties: lowest index
    err = float((d2.cpu().double() - rd).abs().max())
    bar = float(5 * U * rd.max() + 1e-12)
    _report("chamfer_d2", case=label, P=a.shape[0], Q=b.shape[0], max_err=err, bar=bar, unclear=int((~clear).sum()))
    assert err <= bar, (err, bar)
    return d2.cpu(), idx.cpu()


@pytest.mark.parametrize("P,Q", [(1, 1), (255, 511), (257, 512), (300, 513), (1000, 1025)])
def test_nearest_neighbours_partial_blocks_and_splits(lib_built, P, Q):
    g = torch.Generator().manual_seed(P + Q)
    a, b = torch.randn(P, 3, generator=g), torch.randn(Q, 3, generator=g)
    if Q > 20:
        b[Q - 1] = b[3]                         # a duplicate in the last (partial) split: the lower index wins
        a[0] = b[3]
    d2, idx = _nn_check(a, b, "random")
    if Q > 20:
        assert int(idx[0]) == 3 and float(d2[0]) == 0.0


def test_nearest_neighbours_ties(lib_built):
    g = torch.Generator().manual_seed(8)
    # a tie across two splits: b[512] == b[0] and a query on top of it -> index 0
    a, b = torch.randn(300, 3, generator=g), torch.randn(513, 3, generator=g)
    b[512] = b[0]
    a[299] = b[0]
    a[7] = b[0] + torch.tensor([0.01, 0.0, 0.0])                         # not on top of it: the same distance to both copies
    d2, idx = _nn_check(a, b, "tie_across_splits")
    assert int(idx[299]) == 0 and float(d2[299]) == 0.0 and int(idx[7]) == 0
    # all of b identical: every distance ties inside a split and across splits -> index 0 for every query
    b = torch.randn(1, 3, generator=g).repeat(1025, 1)
    d2, idx = _nn_check(a, b, "all_identical")
    assert int(idx.abs().max()) == 0


def test_nearest_neighbours_offset_coordinates(lib_built):
    """Both sets 1e3 away from the origin: the kernel subtracts before it squares, and the difference of two fp32 values in
    [512, 1024) that are less than 16 apart is exact -- the same relative bar holds."""
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(300, 3, generator=g) + 1e3, torch.randn(513, 3, generator=g) + 1e3
    _nn_check(a, b, "offset_1e3")


def test_nearest_neighbours_empty_query_set(lib_built):
    from texgs import uvmap
    d2, idx = uvmap.nearest_neighbours(torch.zeros(0, 3, device=DEV), torch.randn(513, 3).to(DEV))
    torch.cuda.synchronize()
    assert d2.shape == (0,) and idx.shape == (0,) and d2.dtype == torch.float32 and idx.dtype == torch.int64


def test_nearest_neighbours_non_finite_inputs(lib_built):
    """"no finite distance -> d2 = NaN, idx = 0" (include/texgs.h), and a non-finite row is an ordinary value that loses every
    comparison: it changes nothing for its neighbours"""
    from texgs import uvmap
    g = torch.Generator().manual_seed(10)
    a, b = torch.randn(300, 3, generator=g), torch.randn(1025, 3, generator=g)
    d2_0, idx_0 = _nn_check(a, b, "finite")
    nan, inf = float("nan"), float("inf")

    # a query row with a NaN: NaN and index 0 for it, the other queries bit for bit as before
    a2 = a.clone()
    a2[5, 1] = nan
    a2[299] = nan
    d2, idx = (t.cpu() for t in uvmap.nearest_neighbours(a2.to(DEV), b.to(DEV)))
    bad = torch.zeros(300, dtype=torch.bool)
    bad[[5, 299]] = True
    assert bool(torch.isnan(d2[bad]).all()) and int(idx[bad].abs().max()) == 0
    assert torch.equal(d2[~bad], d2_0[~bad]) and torch.equal(idx[~bad], idx_0[~bad])

    # reference rows with NaN or +-inf are never chosen: the result is the brute force over the finite rows, original indices
    b2 = b.clone()
    b2[0, 0] = nan
    b2[int(idx_0[17])] = nan                    # a row that was somebody's nearest neighbour
    b2[100, 2] = inf
    b2[511] = -inf
    b2[512, 1] = -inf
    b2[1024] = torch.tensor([inf, -inf, nan])
    finite = torch.isfinite(b2).all(dim=1)
    keep = finite.nonzero()[:, 0]
    d2, idx = (t.cpu() for t in uvmap.nearest_neighbours(a.to(DEV), b2.to(DEV)))
    rd, ri, gap = _brute(a.double(), b2[keep].double())
    clear = gap > 1e-6 * rd + 1e-30
    assert bool(finite[idx].all())
    assert torch.equal(idx[clear], keep[ri][clear])
    assert float((d2.double() - rd).abs().max()) <= float(5 * U * rd.max() + 1e-12)

    # nothing finite in b: NaN and index 0 for every query
    b3 = b.clone()
    b3[:400, 0] = nan
    b3[400:800, 1] = inf
    b3[800:, 2] = -inf
    d2, idx = (t.cpu() for t in uvmap.nearest_neighbours(a.to(DEV), b3.to(DEV)))
    assert bool(torch.isnan(d2).all()) and int(idx.abs().max()) == 0


@pytest.mark.parametrize("single", [False, True])
def test_chamfer_partial_blocks_and_splits(lib_built, single):
    """chamfer_distance at P = 300, Q = 513 (a partial block and a partial split in either direction): loss and gradients against
    the float64 recomputation with the kernel's indices, the bars of test_chamfer_against_brute_force"""
    from texgs import uvmap
    g = torch.Generator().manual_seed(12)
    x, y = torch.randn(300, 3, generator=g), torch.randn(513, 3, generator=g)
    y[512] = y[0]
    x[:20] = y[200:220]                         # zero distances
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss, none = uvmap.chamfer_distance(xd[None], yd[None], single_directional=single)
    assert none is None
    loss.backward()
    _, ix = _nn_check(x, y, "chamfer_x_to_y")
    _, iy = _nn_check(y, x, "chamfer_y_to_x")
    xa, ya = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ref = ((xa - ya[ix]) ** 2).sum(-1).mean()
    if not single:
        ref = ref + ((ya - xa[iy]) ** 2).sum(-1).mean()
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    assert _rel(xd.grad, xa.grad) < 1e-5, _rel(xd.grad, xa.grad)
    assert _rel(yd.grad, ya.grad) < 1e-5, _rel(yd.grad, ya.grad)
