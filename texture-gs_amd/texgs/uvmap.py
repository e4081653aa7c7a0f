"""The UV-map stage (stage 2 of Texture-GS, models/uv_map_gaussian3d.py:167-238) without tiny-cuda-nn or pytorch3d.

* `HashGridEncoding`: tiny-cuda-nn's multiresolution "HashGrid" encoding (models/modules/utils.py:5-29; F = 4 features per
  level), forward and backward as HIP kernels (csrc/uvmap.hip).  The index rules are restated from tiny-cuda-nn's published grid
  encoding (include/texgs.h) and are UNPINNED against the package, like `uvnet.unpack_tcnn_params`.
* `InvUVNet`: models/modules/uv_net.py:38-85 -- sphere point -> xyz: hash grid, 32 -> 128 -> 128, relu(. + emb),
  128 -> 128 -> 128 -> 3, optional `* xyz_scale + xyz_offset`.  The MLP is bias-free (tiny-cuda-nn's FullyFusedMLP; a 32-wide
  input has no padded column to carry a bias) and runs as fp32 torch GEMMs with a hand-written backward whose weight gradients
  are chunked (`uvnet._tn`).  `load_reference_state` reads the tiny-cuda-nn state every shipped config writes.
* `chamfer_distance`: pytorch3d.loss.chamfer_distance as the reference calls it (batch 1, no lengths / normals, mean point
  reduction, squared L2); the nearest-neighbour search is a HIP kernel.
* `depth2world` and `uv_map_loss`: the stage-2 loss terms Linv, Lchamfer, Lpatch_chamfer and Linv2, term for term.

No CPU fallback: the kernels raise on CPU tensors (tests/hashgrid_ref.py holds the float64 statement the tests compare against).
"""
import ctypes as C
import warnings
from dataclasses import dataclass

import torch
from torch import nn
import torch.nn.functional as F

from . import _lib
from .losses import depth2world      # (models/uv_map_gaussian3d.py:155-165 is the same function as texture_gaussian3d.py:299-309)
from .uvnet import HIDDEN, _tn, unpack_tcnn_params

# configs/uv_map.yaml inv_uv_net_cfg.pre_mlp_cfg.hash_grid_cfg + the constants of models/modules/utils.py:13-14
SHIPPED_GRID = dict(n_levels=8, n_features=4, log2_hashmap_size=12, base_resolution=16.0, per_level_scale=1.447)


def _grid_struct(grid):
    return _lib.HashGridStruct(int(grid["n_levels"]), int(grid["n_features"]), int(grid["log2_hashmap_size"]),
                               float(grid["base_resolution"]), float(grid["per_level_scale"]))


def hashgrid_levels(**grid):
    """The level table of a grid (host arithmetic of the library): dict of per-level `scale`, `res`, `size`, `offset` (rows) and
    `n_params` (floats).  Raises ValueError for an unsupported grid (F != 4, more than 16 levels, ...)."""
    g = dict(SHIPPED_GRID, **grid)
    lib = _lib.load()
    L = int(g["n_levels"])
    n = max(L, 1)
    scale, res, size, off = (C.c_float * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)(), (C.c_uint32 * n)()
    total = C.c_uint32(0)
    st = _grid_struct(g)
    if lib.texgs_hashgrid_levels(C.byref(st), scale, res, size, off, C.byref(total)) != 0:
        raise ValueError(lib.texgs_last_error().decode())
    return dict(scale=list(scale)[:L], res=list(res)[:L], size=list(size)[:L], offset=list(off)[:L], n_params=int(total.value))


def _need_cuda(what, *ts):
    for t in ts:
        if t.device.type != "cuda":
            raise RuntimeError(f"{what} runs on an AMD GPU; there is no CPU fallback")


def _aligned(t):
    """detached, contiguous fp32 whose data starts on a 16-byte boundary (the kernels read rows as float4); a misaligned view
    (a storage offset that is not a multiple of 4 floats) is copied"""
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _check_grid_args(x, params, grid):
    """The C ABI takes bare pointers: the sizes it will index are checked here, before any launch."""
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"x must be [N, 3], got {tuple(x.shape)}")
    n = hashgrid_levels(**grid)["n_params"]
    if params.dim() != 1 or params.numel() != n:
        raise ValueError(f"hash-grid parameters: expected a flat tensor of {n} values for {grid}, got shape {tuple(params.shape)}")
    if x.device != params.device:
        raise ValueError(f"x is on {x.device}, the parameters on {params.device}")


class _HashGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, grid):
        lib = _lib.load()
        _check_grid_args(x, params, grid)
        _need_cuda("the hash-grid encoding", x, params)
        x = _aligned(x)
        params = _aligned(params)
        st = _grid_struct(grid)
        N = x.shape[0]
        enc = torch.empty(N, int(grid["n_levels"]) * _lib.HASHGRID_FEATURES, dtype=torch.float32, device=x.device)
        with _lib.on(x.device) as stream:
            _lib.call(lib.texgs_hashgrid_forward, C.byref(st), params.data_ptr(), x.data_ptr(), N, enc.data_ptr(), stream)
        ctx.grid = grid
        ctx.save_for_backward(x, params)
        return enc

    @staticmethod
    def backward(ctx, g):
        x, params = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_p):
            return None, None, None
        lib = _lib.load()
        st = _grid_struct(ctx.grid)
        N = x.shape[0]
        g = _aligned(g)
        d_p = torch.zeros_like(params) if need_p else None
        d_x = torch.empty_like(x) if need_x else None
        with _lib.on(x.device) as stream:
            temp = torch.empty(max(1, lib.texgs_hashgrid_backward_temp_bytes(C.byref(st), N)) if need_x else 1, dtype=torch.uint8,
                               device=x.device)
            p = _lib.ptr
            _lib.call(lib.texgs_hashgrid_backward, C.byref(st), p(params), p(x), p(g), N, p(d_p), p(d_x), p(temp), stream)
        return d_x, d_p, None


def hashgrid_encode(x, params, grid=None):
    """enc [N, L*4] of points x [N, 3] (not clamped), differentiable w.r.t. x and params."""
    grid = dict(SHIPPED_GRID, **(grid or {}))
    return _HashGrid.apply(x, params, grid)


class HashGridEncoding(nn.Module):
    """tiny-cuda-nn `Encoding(3, {"otype": "HashGrid", ...})`: one flat fp32 parameter vector `params` (levels back to back,
    4 features per table row), initialised uniform in [-1e-4, 1e-4] as tiny-cuda-nn does."""

    def __init__(self, **grid):
        super().__init__()
        self.grid = dict(SHIPPED_GRID, **grid)
        lv = hashgrid_levels(**self.grid)
        self.n_params = lv["n_params"]
        self.n_output_dims = int(self.grid["n_levels"]) * _lib.HASHGRID_FEATURES
        self.params = nn.Parameter(torch.empty(self.n_params).uniform_(-1e-4, 1e-4))

    def forward(self, x):
        return _HashGrid.apply(x, self.params, self.grid)


class _InvMLP(torch.autograd.Function):
    """relu(relu(enc W1^T) W2^T + emb) -> 128 -> 128 -> 3, bias-free, fp32 GEMMs; weight gradients as chunked a^T b."""

    @staticmethod
    def forward(ctx, enc, emb, W1, W2, W3, W4, W5):
        h1 = (enc @ W1.t()).clamp_min_(0)
        a = (h1 @ W2.t() + emb).clamp_min_(0)
        h2 = (a @ W3.t()).clamp_min_(0)
        h3 = (h2 @ W4.t()).clamp_min_(0)
        out = h3 @ W5.t()
        ctx.save_for_backward(enc, W1, W2, W3, W4, W5, h1, a, h2, h3)
        return out

    @staticmethod
    def backward(ctx, do):
        enc, W1, W2, W3, W4, W5, h1, a, h2, h3 = ctx.saved_tensors
        need = ctx.needs_input_grad
        do = do.contiguous()
        dW5 = _tn(do, h3) if need[6] else None
        d4 = (do @ W5) * (h3 > 0)
        dW4 = _tn(d4, h2) if need[5] else None
        d3 = (d4 @ W4) * (h2 > 0)
        dW3 = _tn(d3, a) if need[4] else None
        d2 = (d3 @ W3) * (a > 0)
        dW2 = _tn(d2, h1) if need[3] else None
        demb = d2.sum(0) if need[1] else None
        d_enc = dW1 = None
        if need[0] or need[2]:
            d1 = (d2 @ W2) * (h1 > 0)
            dW1 = _tn(d1, enc) if need[2] else None
            d_enc = d1 @ W1 if need[0] else None
        return d_enc, demb, dW1, dW2, dW3, dW4, dW5


def _emb_vector(emb):
    if isinstance(emb, nn.Embedding):           # the reference's geo_emb = nn.Embedding(1, 128), squeezed (uv_map_gaussian3d.py:180)
        return emb.weight[0]
    return emb.reshape(-1)


class InvUVNet(nn.Module):
    """models/modules/uv_net.py:38-85 with the hash-grid pre-MLP every shipped config uses (configs/uv_map*.yaml)."""

    def __init__(self, xyz_offset=None, xyz_scale=None, n_sample_points=2048, patch_scale=8, emb_dim=HIDDEN, grid=None):
        super().__init__()
        self.encoding = HashGridEncoding(**(grid or {}))
        self.pre_mlp = nn.Sequential(nn.Linear(self.encoding.n_output_dims, HIDDEN, bias=False), nn.ReLU(),
                                     nn.Linear(HIDDEN, emb_dim, bias=False))
        self.mlp = nn.Sequential(nn.Linear(emb_dim, HIDDEN, bias=False), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN, bias=False), nn.ReLU(),
                                 nn.Linear(HIDDEN, 3, bias=False))
        self.n_sample_points = n_sample_points
        self.patch_scale = patch_scale
        self.register_buffer("xyz_offset", None if xyz_offset is None else torch.as_tensor(xyz_offset, dtype=torch.float32), persistent=False)
        self.register_buffer("xyz_scale", None if xyz_scale is None else torch.as_tensor(xyz_scale, dtype=torch.float32), persistent=False)
        self.tcnn_layout_unpinned = False       # set by load_reference_state (tiny-cuda-nn's flat layouts)

    def _weights(self):
        return [self.pre_mlp[0].weight, self.pre_mlp[2].weight, self.mlp[0].weight, self.mlp[2].weight, self.mlp[4].weight]

    def load_reference_state(self, state):
        """A reference `inv_uv_net.state_dict()` of the tiny-cuda-nn form (`pre_mlp.0.params` = the hash-grid table,
        `pre_mlp.1.params` = the 32 -> 128 -> 128 FullyFusedMLP, `mlp.params` = 128 -> 128 -> 128 -> 3), fp16 or fp32, or this
        module's own state_dict."""
        if "pre_mlp.0.params" in state and "pre_mlp.1.params" in state and "mlp.params" in state:
            table = state["pre_mlp.0.params"].detach().reshape(-1)
            n = self.encoding.n_params
            if table.numel() != n:
                raise ValueError(f"hash-grid encoding: expected {n} parameters for {self.encoding.grid}, got {table.numel()}")
            pre = unpack_tcnn_params(state["pre_mlp.1.params"], self.encoding.n_output_dims, HIDDEN, 1)
            mlp = unpack_tcnn_params(state["mlp.params"], HIDDEN, 3, 2)
            with torch.no_grad():
                self.encoding.params.copy_(table.to(torch.float32))
                for w, (src, b) in zip(self._weights(), pre + mlp):
                    assert b is None
                    w.copy_(src)
            self.tcnn_layout_unpinned = True
            warnings.warn("InvUVNet weights were read from tiny-cuda-nn's flat HashGrid / FullyFusedMLP parameter tensors.  Those "
                          "layouts are restated from the published source and are UNPINNED here (tiny-cuda-nn cannot be installed "
                          "in the build container, no fixture produced by it exists): check the inverse map against the reference "
                          "before trusting the checkpoint (module.tcnn_layout_unpinned is set).", RuntimeWarning, stacklevel=2)
            return self
        self.load_state_dict(state)
        self.tcnn_layout_unpinned = False
        return self

    def forward(self, uv, emb):
        x = uv / 2 + 0.5
        enc = self.encoding(x)
        out = _InvMLP.apply(enc, _emb_vector(emb).to(torch.float32), *self._weights())
        if self.xyz_offset is not None and self.xyz_scale is not None:
            out = out * self.xyz_scale.to(out) + self.xyz_offset.to(out)
        return out

    # ---- samples on the unit sphere (uv_net.py:49-68) ----
    def sample(self, n_sample_points=None, device="cuda", generator=None):
        n = self.n_sample_points if n_sample_points is None else n_sample_points
        gdev = generator.device if generator is not None else "cpu"
        with torch.no_grad():
            points = torch.randn(n, 3, generator=generator, device=gdev).to(device).float()
            return F.normalize(points, dim=-1)

    def patch_sample(self, n_sample_points=None, device="cuda", generator=None):
        n = self.n_sample_points if n_sample_points is None else n_sample_points
        gdev = generator.device if generator is not None else "cpu"
        with torch.no_grad():
            direction = F.normalize(torch.randn(3, generator=generator, device=gdev).to(device).float(), dim=0)
            points = F.normalize(torch.randn(n * self.patch_scale, 3, generator=generator, device=gdev).to(device).float(), dim=-1)
            _, idx = torch.topk(torch.sum(points * direction, dim=-1), k=n)
            return points[idx].contiguous()


# ---- chamfer distance ----------------------------------------------------------------------------------------------------
def nearest_neighbours(a, b):
    """(d2 f32[P], idx int64[P]): the nearest b_j of every a_i, squared L2, the lowest j on ties.  HIP kernel."""
    lib = _lib.load()
    if a.dim() != 2 or a.shape[1] != 3 or b.dim() != 2 or b.shape[1] != 3:
        raise ValueError(f"nearest_neighbours: expected [P, 3] and [Q, 3], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"nearest_neighbours: the point sets are on {a.device} and {b.device}")
    _need_cuda("chamfer_distance", a, b)
    a = a.detach().to(torch.float32).contiguous()
    b = b.detach().to(torch.float32).contiguous()
    P, Q = a.shape[0], b.shape[0]
    if Q == 0:
        raise ValueError("chamfer_distance: the other point set is empty")
    d2 = torch.empty(P, dtype=torch.float32, device=a.device)
    idx = torch.empty(P, dtype=torch.int32, device=a.device)
    with _lib.on(a.device) as stream:
        temp = torch.empty(max(1, lib.texgs_chamfer_nn_temp_bytes(P)), dtype=torch.uint8, device=a.device)
        _lib.call(lib.texgs_chamfer_nn, a.data_ptr(), P, b.data_ptr(), Q, d2.data_ptr(), idx.data_ptr(), temp.data_ptr(), stream)
    return d2, idx.long()


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, single_directional):
        dx, ix = nearest_neighbours(x, y)
        loss = dx.mean()
        iy = None
        if not single_directional:
            dy, iy = nearest_neighbours(y, x)
            loss = loss + dy.mean()
        ctx.single = single_directional
        ctx.save_for_backward(x, y, ix, iy if iy is not None else ix)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y, ix, iy = ctx.saved_tensors
        P, Q = x.shape[0], y.shape[0]
        xf, yf = x.detach().float(), y.detach().float()
        rx = (2.0 / P) * (xf - yf[ix]) * g                   # d cham_x / d x_i
        gx = rx.clone()
        gy = torch.zeros_like(yf).index_add_(0, ix, -rx)
        if not ctx.single:
            ry = (2.0 / Q) * (yf - xf[iy]) * g               # d cham_y / d y_j
            gy += ry
            gx.index_add_(0, iy, -ry)
        return (gx.to(x.dtype) if ctx.needs_input_grad[0] else None,
                gy.to(y.dtype) if ctx.needs_input_grad[1] else None, None)


def chamfer_distance(x, y, single_directional=False):
    """pytorch3d.loss.chamfer_distance(x, y[, single_directional]) as models/uv_map_gaussian3d.py:196-216 calls it: x [1, P, 3],
    y [1, Q, 3]; mean over points of the squared distance to the nearest neighbour, both directions summed (or x -> y only).
    Returns (loss, None).  Gradients reach x and y."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[-1] != 3 or y.shape[-1] != 3:
        raise ValueError(f"expected [1, P, 3] and [1, Q, 3], got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[0] != 1 or y.shape[0] != 1:
        raise ValueError("chamfer_distance supports batch size 1 only (what the reference uses)")
    return _Chamfer.apply(x[0], y[0], bool(single_directional)), None


# ---- stage-2 losses --------------------------------------------------------------------------------------------------------
@torch.no_grad()
def render_depth_alpha(settings, means3D, opacities, scales, rotations):
    """The stage-2 render (uv_map_gaussian3d.py:171-176): the untextured diff_gauss forward with colors_precomp = 0, no graph
    (stage 2 freezes the Gaussians).  -> (depth [1, H, W], alpha [1, H, W])."""
    import diff_gauss
    out = diff_gauss.GaussianRasterizer(settings)(means3D=means3D, means2D=None, opacities=opacities,
                                                  colors_precomp=torch.zeros_like(means3D), scales=scales, rotations=rotations)
    return out[1], out[3]


@dataclass
class UVMapLossCfg:
    """The loss weights of configs/uv_map.yaml (a term with weight 0 is off; the caller applies the *_range schedules)."""
    lambda_inverse: float = 1.0
    lambda_chamfer: float = 1.0
    lambda_patch_chamfer: float = 0.0
    lambda_inverse2: float = 1.0


def uv_map_loss(depth, alpha, full_proj_transform, znear, zfar, uv_net, inv_uv_net, geo_emb, pcd, cfg=None, generator=None,
                world_xyz=None):
    """One stage-2 loss, term for term with models/uv_map_gaussian3d.py:167-232 (without the render and loss.backward()).

    depth, alpha: the untextured render [1, H, W] (or [H, W]) of the frozen Gaussians; full_proj_transform, znear, zfar: its
    camera; uv_net: texgs.uvnet.UVNet (evaluated by the fused kernel, so Linv2 reaches the inverse net through J^T g);
    inv_uv_net: InvUVNet; geo_emb: nn.Embedding(1, 128) or a [128] tensor; pcd [Q, 3]: the target point cloud; cfg: UVMapLossCfg,
    a dict or any object with the lambda_* attributes.  Returns (loss, stats).

    world_xyz (opt-in): f32 [M, 3], the surface points of this render, e.g. `texgs.surface.surface_points(...).xyz`.  When given,
    these rows are used instead of the torch unprojection and selection of uv_map_gaussian3d.py:180-183 (depth, alpha and the
    camera are then not read); the default path is unchanged.

    Deviation: the reference's Linv2 branch calls `sample(depth.device)` (:223), passing the device as the point count; that
    line only runs with chamfer off.  Here it samples n_sample_points points."""
    cfg = UVMapLossCfg() if cfg is None else cfg
    lam = (lambda k: float(cfg.get(k, 0.0) or 0.0)) if isinstance(cfg, dict) else (lambda k: float(getattr(cfg, k, 0.0) or 0.0))
    emb = _emb_vector(geo_emb)
    dev = depth.device
    if world_xyz is None:
        d = depth.reshape(depth.shape[-2], depth.shape[-1])
        world_xyz = depth2world(d, full_proj_transform, zfar, znear)
        valid = alpha.reshape(-1) > 0.5
        world_xyz = world_xyz.reshape(-1, 3)[valid].contiguous().detach()
    else:
        if not torch.is_tensor(world_xyz):
            raise TypeError(f"world_xyz must be a torch.Tensor, got {type(world_xyz).__name__}")
        if world_xyz.dim() != 2 or world_xyz.shape[1] != 3 or world_xyz.dtype != torch.float32:
            raise ValueError(f"world_xyz must be float32 [M, 3], got {world_xyz.dtype} {tuple(world_xyz.shape)}")
        world_xyz = world_xyz.contiguous().detach()
    uv, _ = uv_net.uvs_and_jacobian_with_grad(world_xyz, emb)

    loss = torch.zeros((), dtype=torch.float32, device=dev)
    stats = {}
    if lam("lambda_inverse"):
        inv_xyz = inv_uv_net(uv, emb)
        Linv = ((world_xyz - inv_xyz) ** 2).sum(-1).mean()
        loss = loss + lam("lambda_inverse") * Linv
        stats["Linv"] = Linv
    sample_uvs, sample_inv_xyzs = None, None
    if lam("lambda_chamfer"):
        sample_uvs = inv_uv_net.sample(device=dev, generator=generator)
        sample_inv_xyzs = inv_uv_net(sample_uvs, emb)
        Lchamfer, _ = chamfer_distance(sample_inv_xyzs.unsqueeze(0), pcd.unsqueeze(0))
        loss = loss + lam("lambda_chamfer") * Lchamfer
        stats["Lchamfer"] = Lchamfer
    if lam("lambda_patch_chamfer"):
        if sample_uvs is None:
            sample_uvs = inv_uv_net.patch_sample(device=dev, generator=generator)
        if sample_inv_xyzs is None:
            sample_inv_xyzs = inv_uv_net(sample_uvs, emb)
        Lpatch, _ = chamfer_distance(sample_inv_xyzs.unsqueeze(0), pcd.unsqueeze(0), single_directional=True)
        loss = loss + lam("lambda_patch_chamfer") * Lpatch
        stats["Lpatch_chamfer"] = Lpatch
    if lam("lambda_inverse2"):
        if sample_uvs is None:
            sample_uvs = inv_uv_net.sample(device=dev, generator=generator)
        if sample_inv_xyzs is None:
            sample_inv_xyzs = inv_uv_net(sample_uvs, emb)
        sample_inv_uvs, _ = uv_net.uvs_and_jacobian_with_grad(sample_inv_xyzs, emb)
        Linv2 = ((sample_inv_uvs - sample_uvs) ** 2).sum(-1).mean()
        loss = loss + lam("lambda_inverse2") * Linv2
        stats["Linv2"] = Linv2
    stats["total_loss"] = loss
    return loss, stats
