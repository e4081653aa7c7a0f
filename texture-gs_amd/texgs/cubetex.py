"""Seamless cubemap sampling without nvdiffrast (csrc/cubetex.hip): the one function of it that Texture-GS uses,
`dr.texture(..., boundary_mode='cube')`.

* `cube_sample`: texture [6, R, R, C] (faces +x, -x, +y, -y, +z, -z, channels last) at directions [..., 3] of any length, filter
  `linear` or `nearest`, differentiable.
* `latlong_dirs`, `cubemap_to_latlong`: NVDIFFREC/util.py:119-133.  `sphere_map`: models/texture_gaussian3d.py:446-449 in one launch
  (sh02rgb is applied to every tap in the kernel; no RGB copy of the texture and no direction tensor is written).
* `chessboard_texture`: models/uv_map_gaussian3d.py:249-260.

The face is the dominant axis and col = (sc/ma + 1) R/2 - 0.5 as in the rasterizer (texel centres at (i + 0.5)/R;
tests/golden/cube.npz pins the convention).  `linear` takes the four bilinear taps; a tap one texel outside the face reads the face
across that edge, and the tap that would lie past a cube corner, where three faces meet and no fourth texel exists, is dropped and
the other three weights are divided by their sum.  nvdiffrast's documentation promises only that `boundary_mode='cube'` filters
seamlessly across the edges; which texel a crossing tap reads and, above all, the corner rule (drop and renormalise) are this
project's ASSUMPTION about it.  All of it is UNPINNED against the package, which has no ROCm build to compare with
(tests/cubetex_ref.py holds the statement).

A zero or non-finite direction gives a zero row and zero gradients, decided in the kernel without a host synchronisation.  The
texture gradient is a scatter of fp32 atomic adds: its last bits vary from run to run.

No CPU fallback: the kernels raise on CPU tensors.  The C entry points take bare pointers, so every argument is checked here,
before any launch.
"""
import math

import torch

from . import _lib

FILTERS = {"linear": 0, "nearest": 1}       # TEXGS_CUBE_LINEAR, TEXGS_CUBE_NEAREST


def _check_texture(texture, what):
    if not isinstance(texture, torch.Tensor):
        raise TypeError(f"{what}: texture must be a torch.Tensor, got {type(texture).__name__}")
    if texture.dtype != torch.float32:
        raise ValueError(f"{what}: texture must be float32, got {texture.dtype}")
    if texture.dim() != 4 or texture.shape[0] != 6:
        raise ValueError(f"{what}: texture must be [6, R, R, C], got {tuple(texture.shape)}")
    if texture.shape[1] != texture.shape[2]:
        raise ValueError(f"{what}: texture faces must be square, got {tuple(texture.shape)}")
    if texture.shape[1] < 2:
        raise ValueError(f"{what}: texture needs R >= 2, got R = {texture.shape[1]}")
    if texture.shape[3] < 1:
        raise ValueError(f"{what}: texture needs C >= 1 channels, got {tuple(texture.shape)}")
    if texture.numel() >= 2 ** 31:
        raise ValueError(f"{what}: texture holds {texture.numel()} values; the library indexes them with 31 bits")


def _check_dirs(dirs, what):
    if not isinstance(dirs, torch.Tensor):
        raise TypeError(f"{what}: dirs must be a torch.Tensor, got {type(dirs).__name__}")
    if dirs.dtype != torch.float32:
        raise ValueError(f"{what}: dirs must be float32, got {dirs.dtype}")
    if dirs.dim() < 1 or dirs.shape[-1] != 3:
        raise ValueError(f"{what}: dirs must be [..., 3], got {tuple(dirs.shape)}")
    if dirs.numel() // 3 >= 2 ** 31:
        raise ValueError(f"{what}: dirs holds {dirs.numel() // 3} directions; the library indexes them with 31 bits")


def _check_gpu(what, **tensors):
    """last, as in texgs.points: a wrong shape is reported as such on any device"""
    for name, t in tensors.items():
        if t.device.type != "cuda":
            raise RuntimeError(f"{what}: {name} must be on an AMD GPU; there is no CPU fallback")
    devices = {str(t.device) for t in tensors.values()}
    if len(devices) > 1:
        raise ValueError(f"{what}: the arguments are on different devices: {sorted(devices)}")


def _check_filter(filter, what):
    if filter not in FILTERS:
        raise ValueError(f"{what}: filter must be 'linear' or 'nearest', got {filter!r}")


def _check_resolution(resolution, what):
    try:
        h, w = resolution
    except (TypeError, ValueError):
        raise ValueError(f"{what}: resolution must be (H, W), got {resolution!r}") from None
    for v in (h, w):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{what}: resolution must be two positive ints, got {resolution!r}")
    if h * w >= 2 ** 31:
        raise ValueError(f"{what}: resolution {resolution!r} holds 2^31 pixels or more")
    return h, w


def _forward(texture, dirs, filter, tap_map):
    """texture [6, R, R, C], dirs [N, 3], both contiguous fp32 on one GPU -> [N, C]"""
    lib = _lib.load()
    R, C = texture.shape[1], texture.shape[3]
    n = dirs.shape[0]
    out = torch.empty(n, C, dtype=torch.float32, device=texture.device)
    with _lib.on(texture.device) as stream:
        _lib.call(lib.texgs_cube_sample, texture.data_ptr(), R, C, dirs.data_ptr(), n, FILTERS[filter], int(tap_map), out.data_ptr(), stream)
    return out


class _CubeSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, texture, dirs, filter):
        tex = texture.detach().contiguous()
        d = dirs.detach().reshape(-1, 3).contiguous()
        ctx.save_for_backward(tex, d)
        ctx.filter = filter
        ctx.dirs_shape = dirs.shape
        out = _forward(tex, d, filter, False)
        return out.reshape(dirs.shape[:-1] + (tex.shape[3],))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        tex, d = ctx.saved_tensors
        R, C = tex.shape[1], tex.shape[3]
        n = d.shape[0]
        want_tex = ctx.needs_input_grad[0]
        want_dirs = ctx.needs_input_grad[1] and ctx.filter == "linear"
        g = g_out.reshape(n, C).to(torch.float32).contiguous()
        d_tex = torch.zeros_like(tex) if want_tex else None
        d_dirs = torch.empty_like(d) if want_dirs else None
        if want_tex or want_dirs:
            lib = _lib.load()
            with _lib.on(tex.device) as stream:
                if ctx.filter == "linear":
                    _lib.call(lib.texgs_cube_sample_backward, tex.data_ptr(), R, C, d.data_ptr(), n, g.data_ptr(), _lib.ptr(d_tex),
                              _lib.ptr(d_dirs), stream)
                else:
                    _lib.call(lib.texgs_cube_sample_nearest_backward, R, C, d.data_ptr(), n, g.data_ptr(), d_tex.data_ptr(), stream)
        return d_tex, (d_dirs.reshape(ctx.dirs_shape) if want_dirs else None), None


def cube_sample(texture, dirs, filter="linear"):
    """float32 [..., C]: `texture` [6, R, R, C] at the directions `dirs` [..., 3] (any length).  Gradients flow to both inputs for
    `linear`, to the texture only for `nearest`."""
    _check_texture(texture, "cube_sample")
    _check_dirs(dirs, "cube_sample")
    _check_filter(filter, "cube_sample")
    _check_gpu("cube_sample", texture=texture, dirs=dirs)
    return _CubeSample.apply(texture, dirs, filter)


def latlong_dirs(resolution, device):
    """float32 [H, W, 3], the directions of cubemap_to_latlong (NVDIFFREC/util.py:119-133; its meshgrid is 'ij', so gy runs over
    rows): (sin(th) sin(ph), cos(th), -sin(th) cos(ph)), th = pi gy, ph = pi gx, gy = linspace(1/H, 1 - 1/H, H),
    gx = linspace(-1 + 1/W, 1 - 1/W, W).  Computed in float64 and rounded once, as the fused kernel does."""
    h, w = _check_resolution(resolution, "latlong_dirs")
    gy = torch.linspace(1.0 / h, 1.0 - 1.0 / h, h, dtype=torch.float64, device=device)
    gx = torch.linspace(-1.0 + 1.0 / w, 1.0 - 1.0 / w, w, dtype=torch.float64, device=device)
    gy, gx = torch.meshgrid(gy, gx, indexing="ij")
    st, ct = torch.sin(gy * math.pi), torch.cos(gy * math.pi)
    sp, cp = torch.sin(gx * math.pi), torch.cos(gx * math.pi)
    return torch.stack((st * sp, ct, -st * cp), dim=-1).to(torch.float32)


def _latlong(texture, resolution, tap_map, what):
    _check_texture(texture, what)
    h, w = _check_resolution(resolution, what)
    _check_gpu(what, texture=texture)
    lib = _lib.load()
    tex = texture.detach().contiguous()
    R, C = tex.shape[1], tex.shape[3]
    out = torch.empty(h, w, C, dtype=torch.float32, device=tex.device)
    with _lib.on(tex.device) as stream:
        _lib.call(lib.texgs_cube_latlong, tex.data_ptr(), R, C, h, w, int(tap_map), out.data_ptr(), stream)
    return out


def cubemap_to_latlong(cubemap_rgb, resolution):
    """float32 [H, W, C]: util.cubemap_to_latlong in one launch (the directions are computed in the kernel).  No autograd: compose
    `cube_sample(cubemap, latlong_dirs(...))` for gradients."""
    return _latlong(cubemap_rgb, resolution, False, "cubemap_to_latlong")


def sphere_map(texture_sh0, resolution=(512, 1024)):
    """float32 [H, W, C]: models/texture_gaussian3d.py:446-449, cubemap_to_latlong(sh02rgb(texture)), in one launch: sh02rgb
    (clamp(0.28209479177387814 t + 0.5, 0, 1)) is applied to every tap BEFORE the filter, as the reference does by converting the
    whole texture first.  No autograd."""
    return _latlong(texture_sh0, resolution, True, "sphere_map")


_BOARDS = {}


def _chessboard(resolution, device):
    key = (resolution, str(device))
    if key not in _BOARDS:
        i = torch.arange(resolution, device=device)
        even = ((i[:, None] + i[None, :]) % 2 == 0).repeat_interleave(16, 0).repeat_interleave(16, 1)
        colour = torch.where(even[:, :, None], torch.tensor([0.0, 1.0, 1.0], device=device), torch.tensor([1.0, 0.0, 0.0], device=device))
        _BOARDS[key] = colour[None].expand(6, -1, -1, -1).contiguous()
    return _BOARDS[key]


def chessboard_texture(uv, resolution=6):
    """float32 [npts, 3]: models/uv_map_gaussian3d.py:249-260, the colours of a `resolution` x `resolution` chessboard per face
    (16 texels a cell, cyan where row + column is even, red elsewhere) at the directions uv [npts, 3].  The board is built once per
    device and resolution."""
    if isinstance(resolution, bool) or not isinstance(resolution, int) or resolution < 1:
        raise ValueError(f"chessboard_texture: resolution must be a positive int, got {resolution!r}")
    _check_dirs(uv, "chessboard_texture")
    _check_gpu("chessboard_texture", dirs=uv)
    with torch.no_grad():
        return cube_sample(_chessboard(resolution, uv.device), uv.detach().contiguous()).squeeze()
