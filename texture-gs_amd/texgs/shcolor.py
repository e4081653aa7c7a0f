"""The colour stage on the device (csrc/shcolor.hip, include/texgs_shcolor.h): the `convert_SHs_python` branch of the reference's render
glue (render/render.py:64-68 with utils/sh.py:eval_sh), spherical harmonics of degree 0..4 in the view direction -> `colors_precomp`:

    shs_view = get_features.transpose(1, 2).view(-1, 3, K);   dir_pp = get_xyz - camera_center
    colors_precomp = clamp_min(eval_sh(active_sh_degree, shs_view, dir_pp / dir_pp.norm(dim=1, keepdim=True)) + 0.5, 0.0)

* `sh_colors`        those lines for one camera: one launch forward, one backward (gradients to the coefficients and to xyz).
* `sh_colors_views`  the same for the V cameras of a multi-view step -> [V,N,3]: the coefficient rows are read once, not once per
                     view; one forward launch and one backward launch per 16 views, the views' gradients summed in view order.
* `eval_sh`          the reference's eval_sh alone, with its signature: the caller's directions as given, no +0.5, no clamp.

`features` is one tensor [N,K,3] (what get_features returns) or the pair (features_dc [N,1,3], features_rest [N,K-1,3]), which saves
the reference's torch.cat and the split of its backward: the gradients then go to the two tensors directly.  K is 1, 4, 9, 16 or 25
and (degree + 1)^2 <= K; with a degree below the maximum only the first (degree + 1)^2 coefficients are read, and the others get a
zero gradient.  Degree 4 is one more than the rasterizer's own SH path takes: through `colors_precomp` it works on both rasterizer
modules.

The arithmetic is a bit-exact contract stated in numpy by tests/shcolor_ref.py; the SH evaluation has the reference's operation
order, so `eval_sh` equals the reference's float32 CPU result bit for bit.  The direction is this stage's statement (p / sqrt((px px +
py py) + pz pz), three divisions), one unit in the last place from torch's `norm` in some rows.  A point at the camera centre gives
0 / 0 as in the reference: NaN at degree >= 1.  The camera centre gets NO gradient (the reference's camera_center never requires one):
its slot in the backward is None.

Inputs are float32, contiguous and on the GPU: everything is validated before any library call (TypeError / ValueError), then CPU
tensors raise RuntimeError -- there is no CPU fallback.  Everything runs on torch.cuda.current_stream(); nothing waits on the host.
Once differentiable: a double backward raises.  The inputs' autograd version counters are recorded at the forward, and the backward
raises if one was modified in place in between (it recomputes the forward from them)."""
import ctypes as C

import torch

from . import _lib

ROWS_PER_WORKGROUP = 128        # TEXGS_SH_COLORS_ROWS_PER_WORKGROUP
ROWS_PER_WORKGROUP_DEG4 = 256   # TEXGS_SH_COLORS_ROWS_PER_WORKGROUP_DEG4 (the degree-4 forward)
MAX_VIEWS = 16                  # TEXGS_SH_COLORS_MAX_VIEWS
MAX_DEGREE = 4                  # TEXGS_SH_COLORS_MAX_DEGREE
MODE_COLORS, MODE_EVAL = 0, 1   # TEXGS_SH_COLORS / TEXGS_SH_EVAL
LAYOUT_KC, LAYOUT_CK = 0, 1     # TEXGS_SH_LAYOUT_KC / TEXGS_SH_LAYOUT_CK
COEFFS = (1, 4, 9, 16, 25)

_vp, _i32 = C.c_void_p, C.c_int32


class ShColorViewStruct(C.Structure):
    """ctypes mirror of TexGSShColorView (include/texgs_shcolor.h)"""
    _fields_ = [("campos", _vp), ("colors", _vp)]


class ShColorGradViewStruct(C.Structure):
    """ctypes mirror of TexGSShColorGradView"""
    _fields_ = [("campos", _vp), ("g_colors", _vp)]


class ShColorsStruct(C.Structure):
    """ctypes mirror of TexGSShColors"""
    _fields_ = [("sh", _vp), ("sh_dc", _vp), ("sh_rest", _vp), ("xyz", _vp), ("n", _i32), ("coeffs", _i32), ("degree", _i32),
                ("layout", _i32), ("mode", _i32)]


class ShColorsGradStruct(C.Structure):
    """ctypes mirror of TexGSShColorsGrad"""
    _fields_ = [("sh", _vp), ("sh_dc", _vp), ("sh_rest", _vp), ("xyz", _vp), ("d_sh", _vp), ("d_sh_dc", _vp), ("d_sh_rest", _vp),
                ("d_xyz", _vp), ("n", _i32), ("coeffs", _i32), ("degree", _i32), ("layout", _i32), ("mode", _i32), ("accumulate", _i32)]


MIRRORS = {"TexGSShColorView": ShColorViewStruct, "TexGSShColorGradView": ShColorGradViewStruct, "TexGSShColors": ShColorsStruct,
           "TexGSShColorsGrad": ShColorsGradStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_shcolor.h
SIGNATURES = {
    "texgs_sh_colors_forward": (C.c_int, [C.POINTER(ShColorsStruct), C.POINTER(ShColorViewStruct), _i32, _vp]),
    "texgs_sh_colors_backward": (C.c_int, [C.POINTER(ShColorsGradStruct), C.POINTER(ShColorGradViewStruct), _i32, _vp]),
}
# how often each entry point was called from this layer (tests count them: one per 16 views)
CALLS = {"forward": 0, "backward": 0}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


# ---- validation: everything a launch relies on, before any library call ----
def _check_tensor(name, t, shape_text, ok):
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not ok(t):
        raise ValueError(f"{name} must be {shape_text}, got {tuple(t.shape)}")


def _check_contiguous(name, t):
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_degree(degree, K):
    if isinstance(degree, bool) or not isinstance(degree, int):
        raise TypeError(f"degree must be an int, got {type(degree).__name__}")
    if not 0 <= degree <= MAX_DEGREE:
        raise ValueError(f"degree must be in [0, {MAX_DEGREE}], got {degree}")
    if K not in COEFFS:
        raise ValueError(f"the number of coefficients K must be one of {COEFFS}, got {K}")
    if (degree + 1) ** 2 > K:
        raise ValueError(f"degree {degree} needs {(degree + 1) ** 2} coefficients, the features have K = {K}")


def _check_features(features):
    """-> (sh | None, dc | None, rest | None, N, K)"""
    if isinstance(features, (tuple, list)):
        if len(features) != 2:
            raise ValueError(f"features as a pair must be (features_dc, features_rest), got {len(features)} elements")
        dc, rest = features
        _check_tensor("features_dc", dc, "[N,1,3]", lambda t: t.dim() == 3 and t.shape[1] == 1 and t.shape[2] == 3)
        _check_tensor("features_rest", rest, "[N,K-1,3]", lambda t: t.dim() == 3 and t.shape[2] == 3)
        _check_contiguous("features_dc", dc)
        _check_contiguous("features_rest", rest)
        if dc.shape[0] != rest.shape[0]:
            raise ValueError(f"mismatched N: features_dc has {dc.shape[0]} rows, features_rest has {rest.shape[0]} rows")
        return None, dc, rest, int(dc.shape[0]), 1 + int(rest.shape[1])
    _check_tensor("features", features, "[N,K,3] (or a pair (features_dc, features_rest))", lambda t: t.dim() == 3 and t.shape[2] == 3)
    _check_contiguous("features", features)
    return features, None, None, int(features.shape[0]), int(features.shape[1])


def _check_size(N, K):
    if N * K * 3 >= 2 ** 31:
        raise ValueError(f"N * K * 3 must be below 2^31, got {N} * {K} * 3")


def _need_gpu(what, **tensors):
    """After every other check: the tensors live on one device, and CPU tensors are refused (no fallback)"""
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if dev is None:
            dev, first = t.device, name
        elif t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {first} is on {dev}")
    for name, t in tensors.items():
        if t is not None and t.device.type != "cuda":
            raise RuntimeError(f"texgs.shcolor.{what}: {name} is on {t.device}; it runs on an AMD GPU, there is no CPU fallback")
    return dev


def _refuse_double_backward(what):
    if torch.is_grad_enabled():
        raise RuntimeError(f"texgs.shcolor.{what}: a double backward (create_graph=True) is not supported: the gradient is computed by "
                           "a HIP kernel that has no derivative of its own")


def _check_versions(what, versions):
    for name, t, v in versions:
        if t._version != v:
            raise RuntimeError(f"texgs.shcolor.{what}: {name} was modified in place between the forward and the backward (the backward "
                               "belongs to the values the forward read); clone it before modifying")


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---- the launches (detached tensors in, fresh tensors out) ----
def _forward_raw(dev, sh, dc, rest, xyz, cams, N, K, degree, layout, mode):
    """cams: [V,3] or None (eval) -> [V,N,3]"""
    lib = entry()
    p = _lib.ptr
    V = 1 if cams is None else int(cams.shape[0])
    with _lib.on(dev) as stream:
        out = torch.empty(V, N, 3, dtype=torch.float32, device=dev)
        st = ShColorsStruct(p(sh), p(dc), p(rest), p(xyz), N, K, degree, layout, mode)
        for v0 in range(0, V, MAX_VIEWS):
            count = min(MAX_VIEWS, V - v0)
            recs = (ShColorViewStruct * count)(*[ShColorViewStruct(None if cams is None else cams.data_ptr() + 12 * v,
                                                                   out.data_ptr() + 12 * N * v) for v in range(v0, v0 + count)])
            CALLS["forward"] += 1
            _lib.call(lib.texgs_sh_colors_forward, C.byref(st), recs, count, stream)
    return out


def _backward_raw(dev, sh, dc, rest, xyz, cams, g, N, K, degree, layout, mode, want_sh, want_dc, want_rest, want_xyz):
    """g: [V,N,3] dense -> (d_sh, d_dc, d_rest, d_xyz), None where not wanted"""
    lib = entry()
    p = _lib.ptr
    V = int(g.shape[0])
    with _lib.on(dev) as stream:
        new = lambda like: torch.empty(like.shape, dtype=torch.float32, device=dev)
        d_sh = new(sh) if want_sh else None
        d_dc = new(dc) if want_dc else None
        d_rest = new(rest) if want_rest and K > 1 else None
        d_xyz = new(xyz) if want_xyz else None
        for v0 in range(0, V, MAX_VIEWS):
            count = min(MAX_VIEWS, V - v0)
            recs = (ShColorGradViewStruct * count)(*[ShColorGradViewStruct(None if cams is None else cams.data_ptr() + 12 * v,
                                                                           g.data_ptr() + 12 * N * v) for v in range(v0, v0 + count)])
            st = ShColorsGradStruct(p(sh), p(dc), p(rest), p(xyz), p(d_sh), p(d_dc), p(d_rest), p(d_xyz), N, K, degree, layout, mode,
                                    1 if v0 else 0)
            CALLS["backward"] += 1
            _lib.call(lib.texgs_sh_colors_backward, C.byref(st), recs, count, stream)
        if want_rest and K == 1:
            d_rest = torch.zeros_like(rest)
    return d_sh, d_dc, d_rest, d_xyz


class _ShColors(torch.autograd.Function):
    """(sh | None, dc | None, rest | None, xyz, cams | None) -> [V,N,3]"""

    @staticmethod
    def forward(ctx, sh, dc, rest, xyz, cams, N, K, degree, layout, mode, save, what):
        ctx.set_materialize_grads(False)
        dev = xyz.device
        out = _forward_raw(dev, sh, dc, rest, xyz, cams, N, K, degree, layout, mode)
        ctx.meta = (N, K, degree, layout, mode, what, dev, sh is not None)
        if save:            # (the wrapper decides: grad mode is always off in here; without it no node exists and no backward runs)
            named = (("features", sh), ("features_dc", dc), ("features_rest", rest), ("xyz" if mode == MODE_COLORS else "dirs", xyz),
                     ("campos", cams))
            ctx.versions = [(n, t, t._version) for n, t in named if t is not None]
            ctx.save_for_backward(sh, dc, rest, xyz, cams)
        return out

    @staticmethod
    def backward(ctx, g):
        N, K, degree, layout, mode, what, dev, single = ctx.meta
        _refuse_double_backward(what)
        _check_versions(what, ctx.versions)
        sh, dc, rest, xyz, cams = ctx.saved_tensors
        nig = ctx.needs_input_grad
        want = (single and nig[0], (not single) and nig[1], (not single) and nig[2], nig[3])
        out = [None, None, None, None]
        if any(want) and g is not None and N > 0:
            if g.dtype != torch.float32 or g.dim() != 3 or g.shape[1] != N or g.shape[2] != 3:
                raise ValueError(f"upstream gradient must be float32 [V,{N},3], got {g.dtype} {tuple(g.shape)}")
            out = list(_backward_raw(dev, sh, dc, rest, xyz, cams, g.contiguous(), N, K, degree, layout, mode, *want))
        elif any(want) and g is not None:
            out = [torch.zeros_like(t) if w else None for t, w in zip((sh, dc, rest, xyz), want)]
        return (*out, None, None, None, None, None, None, None, None)


def _colors(what, features, xyz, camposes, degree, views):
    sh, dc, rest, N, K = _check_features(features)
    _check_tensor("xyz", xyz, "[N,3]", lambda t: t.dim() == 2 and t.shape[1] == 3)
    _check_contiguous("xyz", xyz)
    if views:
        _check_tensor("camposes", camposes, "[V,3] with V >= 1", lambda t: t.dim() == 2 and t.shape[1] == 3 and t.shape[0] >= 1)
    else:
        _check_tensor("campos", camposes, "[3] or [1,3]", lambda t: tuple(t.shape) in ((3,), (1, 3)))
    if int(xyz.shape[0]) != N:
        raise ValueError(f"mismatched N: the features have {N} rows, xyz has {int(xyz.shape[0])} rows")
    _check_degree(degree, K)
    _check_size(N, K)
    dev = _need_gpu(what, features=sh, features_dc=dc, features_rest=rest, xyz=xyz, campos=camposes)
    cams = camposes.detach().reshape(-1, 3).contiguous()         # no gradient to the camera centre
    return _ShColors.apply(sh, dc, rest, xyz, cams, N, K, degree, LAYOUT_KC, MODE_COLORS, _wants_grad(sh, dc, rest, xyz), what)


def sh_colors(features, xyz, campos, degree):
    """render.py:64-68 -> colors_precomp f32 [N,3].  features f32 [N,K,3] or the pair (features_dc [N,1,3], features_rest [N,K-1,3]);
    xyz f32 [N,3]; campos f32 [3] (the view's camera_center, on the GPU; it gets no gradient); degree: the active degree, 0..4.
    Differentiable in the features and in xyz: one forward launch, one backward launch."""
    return _colors("sh_colors", features, xyz, campos, degree, False)[0]


def sh_colors_views(features, xyz, camposes, degree):
    """`sh_colors` for the V cameras of one step -> f32 [V,N,3]; row v has the bits of sh_colors(features, xyz, camposes[v], degree).
    The coefficient rows are read once per 16 views, forward and backward; the backward sums the views in the order v = 0..V-1."""
    return _colors("sh_colors_views", features, xyz, camposes, degree, True)


def eval_sh(deg, sh, dirs):
    """The reference's utils/sh.py:eval_sh on the GPU -> f32 [N,3].  sh f32 [N,3,K]: contiguous, or the transposed view
    `features.transpose(1, 2)` of a contiguous [N,K,3] tensor that the reference passes (taken as it lies in memory, without a
    copy); dirs f32 [N,3]: used as given.  No +0.5, no clamp.  Differentiable in both."""
    _check_tensor("sh", sh, "[N,3,K]", lambda t: t.dim() == 3 and t.shape[1] == 3)
    _check_tensor("dirs", dirs, "[N,3]", lambda t: t.dim() == 2 and t.shape[1] == 3)
    _check_contiguous("dirs", dirs)
    N, K = int(sh.shape[0]), int(sh.shape[2])
    if int(dirs.shape[0]) != N:
        raise ValueError(f"mismatched N: sh has {N} rows, dirs has {int(dirs.shape[0])} rows")
    _check_degree(deg, K)
    _check_size(N, K)
    if sh.transpose(1, 2).is_contiguous():
        layout = LAYOUT_KC
    elif sh.is_contiguous():
        layout = LAYOUT_CK
    else:
        raise ValueError("sh must be contiguous [N,3,K] or the transpose(1, 2) of a contiguous [N,K,3] tensor (it is taken without a copy)")
    _need_gpu("eval_sh", sh=sh, dirs=dirs)
    return _EvalSh.apply(sh, dirs, N, K, deg, layout, _wants_grad(sh, dirs))


class _EvalSh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sh, dirs, N, K, degree, layout, save):
        ctx.set_materialize_grads(False)
        dev = dirs.device
        out = _forward_raw(dev, sh, None, None, dirs, None, N, K, degree, layout, MODE_EVAL)[0]
        ctx.meta = (N, K, degree, layout, dev)
        if save:
            ctx.versions = [("sh", sh, sh._version), ("dirs", dirs, dirs._version)]
            ctx.save_for_backward(sh, dirs)
        return out

    @staticmethod
    def backward(ctx, g):
        N, K, degree, layout, dev = ctx.meta
        _refuse_double_backward("eval_sh")
        _check_versions("eval_sh", ctx.versions)
        sh, dirs = ctx.saved_tensors
        want = ctx.needs_input_grad[:2]
        d_sh = d_dirs = None
        if any(want) and g is not None:
            if g.dtype != torch.float32 or tuple(g.shape) != (N, 3):
                raise ValueError(f"upstream gradient must be float32 ({N}, 3), got {g.dtype} {tuple(g.shape)}")
            if N == 0:
                d_sh, d_dirs = (torch.zeros_like(sh) if want[0] else None), (torch.zeros_like(dirs) if want[1] else None)
            else:
                # the gradient of sh in sh's own memory layout: for the transposed view, a [N,K,3] tensor seen through the same transpose
                like = sh.transpose(1, 2) if layout == LAYOUT_KC else sh
                d_like, _, _, d_dirs = _backward_raw(dev, like, None, None, dirs, None, g.contiguous().reshape(1, N, 3), N, K, degree, layout,
                                                     MODE_EVAL, want[0], False, False, want[1])
                if d_like is not None:
                    d_sh = d_like.transpose(1, 2) if layout == LAYOUT_KC else d_like
        return d_sh, d_dirs, None, None, None, None, None
