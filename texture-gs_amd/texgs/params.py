"""The parameter stage on the device (csrc/params.hip, include/texgs_params.h): the first thing every render of the reference does,
turning the stored parameters into the operator's inputs (models/texture_gaussian3d.py):

    get_scaling  = torch.exp(_scaling)          get_rotation = F.normalize(_rotation)          get_opacity = torch.sigmoid(_opacity)
    zero_one_loss(get_opacity)                  lambda_opacity_reg, :370-373
    get_covariance(scaling_modifier)            behind compute_cov3D_python

* `activate`       the three getters in one launch (with `opacity_reg=True` the regulariser rides along: a second one-workgroup
                   launch sums its fp64 partials) and ONE backward launch, however many renders consume the outputs: autograd sums
                   their gradients before this stage's node runs.
* `zero_one_loss`  the regulariser alone, on the opacity PARAMETER (sigmoid inside).
* `covariance`     get_covariance, [N,6] in strip_lowerdiag's order, one launch each way.

The arithmetic is a bit-exact contract stated in numpy by tests/params_ref.py, exp and log included (two fixed polynomials, so a
row's bits do not depend on N, on the row's position or on a math library's version).  Where float32 squares overflow or underflow
the float32 statement holds (`rotations` = q / inf = 0, or q / 1e-12 with n = 0), whatever torch gives there.  `covariance` divides by
the norm without an epsilon, as build_rotation does: a zero quaternion gives a non-finite row.

Inputs are float32, contiguous and on the GPU: everything is validated before any library call (TypeError / ValueError), then CPU
tensors raise RuntimeError -- there is no CPU fallback.  Everything runs on torch.cuda.current_stream(); nothing waits on the host.
Once differentiable: a double backward raises.  The inputs' autograd version counters are recorded at the forward, and the backward
raises if one was modified in place in between (it re-reads the raw rotation through a pointer), as the rasterizer layer does."""
import ctypes as C
import math

import torch

from . import _lib

ROWS_PER_WORKGROUP = 256            # TEXGS_PARAMS_ROWS_PER_WORKGROUP

_vp, _i32, _f32, _size = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


class ParamsActivateStruct(C.Structure):
    """ctypes mirror of TexGSParamsActivate (include/texgs_params.h)"""
    _fields_ = [("scaling", _vp), ("rotation", _vp), ("opacity", _vp), ("scales", _vp), ("rotations", _vp), ("opacities", _vp),
                ("reg", _vp), ("epsilon", _f32), ("n", _i32)]


class ParamsActivateGradStruct(C.Structure):
    """ctypes mirror of TexGSParamsActivateGrad"""
    _fields_ = [("scales", _vp), ("rotation", _vp), ("opacities", _vp), ("g_scales", _vp), ("g_rotations", _vp), ("g_opacities", _vp),
                ("g_reg", _vp), ("d_scaling", _vp), ("d_rotation", _vp), ("d_opacity", _vp), ("epsilon", _f32), ("n", _i32)]


class ParamsCovarianceStruct(C.Structure):
    """ctypes mirror of TexGSParamsCovariance"""
    _fields_ = [("scaling", _vp), ("rotation", _vp), ("cov", _vp), ("scale_modifier", _f32), ("n", _i32)]


class ParamsCovarianceGradStruct(C.Structure):
    """ctypes mirror of TexGSParamsCovarianceGrad"""
    _fields_ = [("scaling", _vp), ("rotation", _vp), ("g_cov", _vp), ("d_scaling", _vp), ("d_rotation", _vp), ("scale_modifier", _f32),
                ("n", _i32)]


MIRRORS = {"TexGSParamsActivate": ParamsActivateStruct, "TexGSParamsActivateGrad": ParamsActivateGradStruct,
           "TexGSParamsCovariance": ParamsCovarianceStruct, "TexGSParamsCovarianceGrad": ParamsCovarianceGradStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_params.h
SIGNATURES = {
    "texgs_params_temp_bytes": (_size, [_i32]),
    "texgs_params_activate": (C.c_int, [C.POINTER(ParamsActivateStruct), _vp, _size, _vp]),
    "texgs_params_activate_backward": (C.c_int, [C.POINTER(ParamsActivateGradStruct), _vp]),
    "texgs_params_covariance": (C.c_int, [C.POINTER(ParamsCovarianceStruct), _vp]),
    "texgs_params_covariance_backward": (C.c_int, [C.POINTER(ParamsCovarianceGradStruct), _vp]),
}
# how often each backward entry point was called from this layer (tests count them: one per backward, however many consumers)
BACKWARD_CALLS = {"activate": 0, "covariance": 0}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


# ---- validation: everything a launch relies on, before any library call ----
def _check_rows(name, t, width, flat_ok=False):
    """t: float32 contiguous [N, width] (or [N] with flat_ok) -> N"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    ok = (t.dim() == 2 and t.shape[1] == width) or (flat_ok and t.dim() == 1)
    if not ok:
        raise ValueError(f"{name} must be [N,{width}]{' or [N]' if flat_ok else ''}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if int(t.shape[0]) >= 2 ** 31:
        raise ValueError(f"{name}: N must be below 2^31, got {int(t.shape[0])}")
    return int(t.shape[0])


def _check_same_rows(**rows):
    if len(set(rows.values())) > 1:
        raise ValueError("mismatched N: " + ", ".join(f"{k} has {v} rows" for k, v in rows.items()))


def _check_number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number, got {type(v).__name__}")
    return float(v)


def _check_epsilon(epsilon):
    epsilon = _check_number("epsilon", epsilon)
    e32 = C.c_float(epsilon).value if math.isfinite(epsilon) else epsilon
    if not (0.0 < e32 < 0.5):
        raise ValueError(f"epsilon must lie in (0, 0.5) as a float32, got {epsilon}")
    return epsilon


def _check_modifier(scale_modifier):
    m = _check_number("scale_modifier", scale_modifier)
    m32 = C.c_float(m).value if math.isfinite(m) else float("nan")
    if not (math.isfinite(m32) and m32 > 0.0):
        raise ValueError(f"scale_modifier must be finite and positive as a float32, got {scale_modifier}")
    return m


def _need_gpu(what, **tensors):
    """After every other check: the tensors live on one device, and CPU tensors are refused (no fallback)"""
    dev = None
    for name, t in tensors.items():
        if dev is None:
            dev, first = t.device, name
        elif t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {first} is on {dev}")
    for name, t in tensors.items():
        if t.device.type != "cuda":
            raise RuntimeError(f"texgs.params.{what}: {name} is on {t.device}; it runs on an AMD GPU, there is no CPU fallback")
        if name == "rotation" and t.data_ptr() % 16:
            raise ValueError("rotation must be 16-byte aligned (a quaternion moves as one 16-byte access)")
    return dev


# ---- the launches (detached tensors in, fresh tensors out) ----
def _activate_raw(dev, scaling, rotation, opacity, want_reg, epsilon):
    lib = entry()
    p = _lib.ptr
    N = int(opacity.shape[0])
    with _lib.on(dev) as stream:
        scales = None if scaling is None else torch.empty_like(scaling)
        rotations = None if rotation is None else torch.empty_like(rotation)
        opacities = torch.empty_like(opacity)
        reg = temp = None
        nbytes = 0
        if want_reg:
            reg = torch.empty((), dtype=torch.float32, device=dev)
            nbytes = lib.texgs_params_temp_bytes(N)
            temp = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        st = ParamsActivateStruct(p(scaling), p(rotation), p(opacity), p(scales), p(rotations), p(opacities), p(reg), epsilon, N)
        _lib.call(lib.texgs_params_activate, C.byref(st), p(temp), nbytes, stream)
    return scales, rotations, opacities, reg


def _grad_in(g, like):
    """An upstream gradient as the kernel reads it: None stays None (a zero gradient), anything else float32 and dense"""
    if g is None:
        return None
    if g.dtype != torch.float32 or g.shape != like.shape:
        raise ValueError(f"upstream gradient must be float32 {tuple(like.shape)}, got {g.dtype} {tuple(g.shape)}")
    return g.contiguous()


def _activate_backward_raw(dev, N, scales, rotation, opacities, g_scales, g_rotations, g_opacities, g_reg, epsilon, want):
    lib = entry()
    p = _lib.ptr
    with _lib.on(dev) as stream:
        d_scaling = torch.empty(N, 3, dtype=torch.float32, device=dev) if want[0] else None
        d_rotation = torch.empty(N, 4, dtype=torch.float32, device=dev) if want[1] else None
        d_opacity = torch.empty_like(opacities) if want[2] else None
        st = ParamsActivateGradStruct(p(scales), p(rotation), p(opacities), p(g_scales), p(g_rotations), p(g_opacities), p(g_reg),
                                      p(d_scaling), p(d_rotation), p(d_opacity), epsilon, N)
        BACKWARD_CALLS["activate"] += 1
        _lib.call(lib.texgs_params_activate_backward, C.byref(st), stream)
    return d_scaling, d_rotation, d_opacity


def _refuse_double_backward(what):
    if torch.is_grad_enabled():
        raise RuntimeError(f"texgs.params.{what}: a double backward (create_graph=True) is not supported: the gradient is computed by a "
                           "HIP kernel that has no derivative of its own")


def _check_versions(what, versions):
    for name, t, v in versions:
        if t._version != v:
            raise RuntimeError(f"texgs.params.{what}: {name} was modified in place between the forward and the backward (the backward "
                               "belongs to the values the forward read); clone it before modifying")


class _Activate(torch.autograd.Function):
    """(scaling | None, rotation | None, opacity) -> the activated tensors that have an input, then reg when asked for"""

    @staticmethod
    def forward(ctx, scaling, rotation, opacity, want_reg, epsilon, save, what):
        ctx.set_materialize_grads(False)
        dev = opacity.device
        scales, rotations, opacities, reg = _activate_raw(dev, scaling, rotation, opacity, want_reg, epsilon)
        ctx.layout = (scaling is not None, rotation is not None, want_reg)
        ctx.epsilon, ctx.what, ctx.dev = epsilon, what, dev
        if save:            # (the wrapper decides: grad mode is always off in here; without it no node exists and no backward runs)
            ctx.versions = [(n, t, t._version) for n, t in (("scaling", scaling), ("rotation", rotation), ("opacity", opacity))
                            if t is not None]
            ctx.save_for_backward(scales, rotation, opacities)
        return tuple(t for t in (scales, rotations, opacities, reg) if t is not None)

    @staticmethod
    def backward(ctx, *grads):
        _refuse_double_backward(ctx.what)
        _check_versions(ctx.what, ctx.versions)
        has_s, has_r, has_reg = ctx.layout
        grads = list(grads)
        g_scales = grads.pop(0) if has_s else None
        g_rotations = grads.pop(0) if has_r else None
        g_opacities = grads.pop(0)
        g_reg = grads.pop(0) if has_reg else None
        scales, rotation, opacities = ctx.saved_tensors
        nig = ctx.needs_input_grad
        want = (has_s and nig[0], has_r and nig[1], nig[2])
        out = [None, None, None]
        if any(want):
            if g_reg is not None:
                g_reg = g_reg.to(torch.float32).reshape(()).contiguous()
            out = _activate_backward_raw(ctx.dev, int(opacities.shape[0]), scales, rotation, opacities,
                                         _grad_in(g_scales, scales) if has_s else None,
                                         _grad_in(g_rotations, rotation) if has_r else None, _grad_in(g_opacities, opacities),
                                         g_reg, ctx.epsilon, want)
        return (*out, None, None, None, None)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def activate(scaling, rotation, opacity, *, opacity_reg=False, epsilon=1e-3):
    """The three getters in one launch -> (scales [N,3], rotations [N,4], opacities shaped like `opacity`), and with
    opacity_reg=True a fourth value: zero_one_loss of the opacities, a 0-dim tensor.

    scaling f32 [N,3], rotation f32 [N,4], opacity f32 [N,1] or [N]: the stored parameters, contiguous, on the GPU.  One autograd
    node and one backward launch whatever the number of consumers; inputs that do not require grad get None; under no_grad nothing
    is saved.  Compute it once per iteration and hand the same tensors to every render of that iteration."""
    N = _check_rows("scaling", scaling, 3)
    Nr = _check_rows("rotation", rotation, 4)
    No = _check_rows("opacity", opacity, 1, flat_ok=True)
    _check_same_rows(scaling=N, rotation=Nr, opacity=No)
    if not isinstance(opacity_reg, bool):
        raise TypeError(f"opacity_reg must be a bool, got {type(opacity_reg).__name__}")
    epsilon = _check_epsilon(epsilon)
    if opacity_reg and N == 0:
        raise ValueError("opacity_reg with N = 0: a mean over nothing")
    _need_gpu("activate", scaling=scaling, rotation=rotation, opacity=opacity)
    return _Activate.apply(scaling, rotation, opacity, opacity_reg, epsilon, _wants_grad(scaling, rotation, opacity), "activate")


def zero_one_loss(opacity_param, epsilon=1e-3):
    """The regulariser on its own: zero_one_loss(sigmoid(opacity_param)), a 0-dim tensor, differentiable in the PARAMETER.  The same
    kernel as `activate(..., opacity_reg=True)`, so the same bits."""
    N = _check_rows("opacity_param", opacity_param, 1, flat_ok=True)
    epsilon = _check_epsilon(epsilon)
    if N == 0:
        raise ValueError("zero_one_loss with N = 0: a mean over nothing")
    _need_gpu("zero_one_loss", opacity_param=opacity_param)
    return _Activate.apply(None, None, opacity_param, True, epsilon, _wants_grad(opacity_param), "zero_one_loss")[1]


class _Covariance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, rotation, modifier, save):
        ctx.set_materialize_grads(False)
        lib = entry()
        dev = scaling.device
        N = int(scaling.shape[0])
        with _lib.on(dev) as stream:
            cov = torch.empty(N, 6, dtype=torch.float32, device=dev)
            st = ParamsCovarianceStruct(_lib.ptr(scaling), _lib.ptr(rotation), _lib.ptr(cov), modifier, N)
            _lib.call(lib.texgs_params_covariance, C.byref(st), stream)
        ctx.modifier, ctx.dev = modifier, dev
        if save:
            ctx.versions = [("scaling", scaling, scaling._version), ("rotation", rotation, rotation._version)]
            ctx.save_for_backward(scaling, rotation)
        return cov

    @staticmethod
    def backward(ctx, g_cov):
        _refuse_double_backward("covariance")
        _check_versions("covariance", ctx.versions)
        scaling, rotation = ctx.saved_tensors
        want = ctx.needs_input_grad[:2]
        if not any(want):
            return None, None, None, None
        lib = entry()
        N = int(scaling.shape[0])
        p = _lib.ptr
        with _lib.on(ctx.dev) as stream:
            if g_cov is not None:
                if g_cov.dtype != torch.float32 or tuple(g_cov.shape) != (N, 6):
                    raise ValueError(f"upstream gradient must be float32 ({N}, 6), got {g_cov.dtype} {tuple(g_cov.shape)}")
                g_cov = g_cov.contiguous()
            d_scaling = torch.empty_like(scaling) if want[0] else None
            d_rotation = torch.empty_like(rotation) if want[1] else None
            st = ParamsCovarianceGradStruct(p(scaling), p(rotation), p(g_cov), p(d_scaling), p(d_rotation), ctx.modifier, N)
            BACKWARD_CALLS["covariance"] += 1
            _lib.call(lib.texgs_params_covariance_backward, C.byref(st), stream)
        return d_scaling, d_rotation, None, None


def covariance(scaling, rotation, scale_modifier=1.0):
    """get_covariance -> f32 [N,6]: (R S)(R S)^T with S = diag(scale_modifier * exp(scaling)) and R from rotation / |rotation|, in
    strip_lowerdiag's order (xx, xy, xz, yy, yz, zz).  Takes the RAW parameters; one launch, and one for the backward, which gives
    gradients to both.  A zero quaternion gives a non-finite row (build_rotation has no epsilon); it is not checked."""
    N = _check_rows("scaling", scaling, 3)
    Nr = _check_rows("rotation", rotation, 4)
    _check_same_rows(scaling=N, rotation=Nr)
    m = _check_modifier(scale_modifier)
    _need_gpu("covariance", scaling=scaling, rotation=rotation)
    return _Covariance.apply(scaling, rotation, m, _wants_grad(scaling, rotation))
