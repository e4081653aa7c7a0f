"""The backward of LPIPS-VGG in the images (csrc/lpips_grad.hip, include/texgs_lpips_grad.h): what makes
`LPIPSVGG(...)(render, gt, normalize=True)` a loss term.

The data gradient of a 3x3 / stride 1 / padding 1 convolution is again such a convolution, with the weights transposed in the channel
axes and flipped in both taps (`transposed_weight`), so texgs.lpips.conv3x3 -- the MFMA implicit GEMM -- runs the thirteen data
gradients unchanged (relu off, no pool, no affine, a zero bias).  Between them stand the two streaming kernels of this module:

* `head_backward`   one tapped layer in ONE launch: the head's gradient in the tapped map, plus the gradient that arrives from the next
                    slice routed through the 2x2 max-pool (to the FIRST maximum of a window in row-major order; an odd last row or
                    column belongs to no window), times the ReLU gate of the convolution that wrote the map.
* `gate`            G = y > 0 ? G : 0 in place: the ReLU of a convolution that is not tapped.

Two rules are deliberate: a pixel whose feature norm is 0 gets a zero head gradient (the derivative of sqrt at 0 is not finite: torch
would return NaN there), and equal maxima of a pool window send the gradient to the first of them.  The weights are constants: no
gradient reaches them.  fp32 only.  `LpipsFunction` is the torch.autograd.Function behind LPIPSVGG.__call__; the chain itself is
LPIPSVGG._forward_grad / _backward_grad.  tests/lpips_grad_ref.py holds the float64 statement.

The ctypes mirror and the signatures of the header live here, as texgs/surface.py keeps those of texgs_surface.h."""
import ctypes as C

import torch

from . import _lib
from . import lpips as L

WRT_FIRST, WRT_PARTNER = 1, 2       # TEXGS_LPIPS_WRT_FIRST / _PARTNER: the bits of `wrt`
MAX_GATE = 2 ** 40                  # texgs_lpips_gate: n below it

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64


class LpipsHeadBackwardStruct(C.Structure):
    """ctypes mirror of TexGSLpipsHeadBackward (include/texgs_lpips_grad.h)"""
    _fields_ = [("f", _vp), ("lin", _vp), ("gbar", _vp), ("g_next", _vp), ("G", _vp), ("P", _i32), ("C", _i32), ("h", _i32), ("w", _i32),
                ("wrt", _i32), ("g_row", _i64), ("g_chan", _i64), ("g_img", _i64)]


MIRRORS = {"TexGSLpipsHeadBackward": LpipsHeadBackwardStruct}
# the entry points' signatures: name -> (restype, argtypes), in the order of include/texgs_lpips_grad.h
SIGNATURES = {
    "texgs_lpips_head_backward": (C.c_int, [C.POINTER(LpipsHeadBackwardStruct), _vp]),
    "texgs_lpips_gate": (C.c_int, [_vp, _vp, _i64, _vp]),
}


def entry():
    """The loaded library with the signatures above applied (on first use)"""
    return _lib.bind(SIGNATURES)


def check_wrt(wrt):
    if wrt not in (1, 2, 3):
        raise ValueError(f"wrt must be 1 (the first images), 2 (their partners) or 3 (both), got {wrt!r}")
    return int(wrt)


def selected(P, wrt):
    """Images of a gradient map: the P that `wrt` selects, or all 2P"""
    return 2 * P if wrt == 3 else P


def transposed_weight(w):
    """w [Cout, Cin, 3, 3] -> the weights of the convolution that is its data gradient: [Cin padded to a multiple of 16 with zero
    rows, Cout, 3, 3], flipped in both taps.  (conv1_1's gradient has 3 channels: 13 of its 16 output planes are zero.)"""
    if not torch.is_tensor(w) or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"w must be [Cout, Cin, 3, 3], got {tuple(getattr(w, 'shape', ()))}")
    wt = w.flip(2, 3).transpose(0, 1)
    rows = -(-wt.shape[0] // 16) * 16
    out = torch.zeros(rows, wt.shape[1], 3, 3, dtype=w.dtype, device=w.device)
    out[:wt.shape[0]] = wt
    return out


def _check_f32(name, t, shape_text, ok, views=False):
    """Shape, dtype and layout of one argument; the devices are looked at last (`_check_gpu`), so that a CPU tensor of the wrong
    shape is refused for its shape"""
    if not torch.is_tensor(t) or not ok(t):
        raise ValueError(f"{name} must be {shape_text}, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_contiguous() and not (views and L._is_plane_view(t)):
        raise ValueError(f"{name} must be contiguous" + (" or a view with adjacent columns and ascending, non-overlapping strides" if views else ""))


def _check_gpu(first, **tensors):
    for name, t in tensors.items():
        if t is not None and t.device.type != "cuda":
            raise RuntimeError(f"{name} must be on an AMD GPU; there is no CPU fallback")
    for name, t in tensors.items():
        if t is not None and t.device != tensors[first].device:
            raise ValueError(f"{name} is on {t.device}, {first} on {tensors[first].device}")


def _head_backward(lib, stream, f_ptr, lin, gbar, g_next_ptr, G_ptr, P, Cn, h, w, wrt, g_strides=(0, 0, 0)):
    st = LpipsHeadBackwardStruct(f_ptr, lin.data_ptr(), gbar.data_ptr(), g_next_ptr, G_ptr, P, Cn, h, w, wrt, *g_strides)
    _lib.call(lib.texgs_lpips_head_backward, C.byref(st), stream)


def _gate(lib, stream, G_ptr, y_ptr, n):
    _lib.call(lib.texgs_lpips_gate, G_ptr, y_ptr, n, stream)


def head_backward(f, lin, gbar, wrt, g_next=None, out=None):
    """One tapped layer's gradient (module docstring): f f32 [2P, C, h, w] (first images, then their partners), lin f32 [C], gbar f32
    [P], g_next f32 [B', C, h // 2, w // 2] or None -> G f32 [B', C, h, w], where B' = P images for wrt = 1 (the first images) or 2
    (the partners) and 2P for wrt = 3.  `out` may be a view into a larger buffer, as conv3x3's.  Enqueues on the current stream."""
    wrt = check_wrt(wrt)
    _check_f32("f", f, "[2P, C, h, w]", lambda t: t.dim() == 4 and t.shape[0] >= 2 and t.shape[0] % 2 == 0)
    P, Cn, h, w = int(f.shape[0]) // 2, int(f.shape[1]), int(f.shape[2]), int(f.shape[3])
    _check_f32("lin", lin, f"[{Cn}]", lambda t: tuple(t.shape) == (Cn,))
    _check_f32("gbar", gbar, f"[{P}]", lambda t: tuple(t.shape) == (P,))
    if not 1 <= Cn <= L.MAX_CHANNELS or h < 1 or w < 1 or h * w >= 2 ** 31 or P > L.MAX_BATCH:
        raise ValueError(f"f of {tuple(f.shape)} is outside the head's limits (C <= {L.MAX_CHANNELS}, h w < 2^31, P <= {L.MAX_BATCH})")
    Bg = selected(P, wrt)
    if g_next is not None:
        if h < 2 or w < 2:
            raise ValueError(f"g_next needs a map of at least 2x2, got {h}x{w}")
        shape = (Bg, Cn, h // 2, w // 2)
        _check_f32("g_next", g_next, f"{list(shape)}", lambda t: tuple(t.shape) == shape)
    if out is not None:
        _check_f32("out", out, f"[{Bg}, {Cn}, {h}, {w}]", lambda t: tuple(t.shape) == (Bg, Cn, h, w), views=True)
    _check_gpu("f", f=f, lin=lin, gbar=gbar, g_next=g_next, out=out)
    if out is None:
        out = torch.empty(Bg, Cn, h, w, dtype=torch.float32, device=f.device)
    lib = entry()
    with _lib.on(f.device) as stream:
        _head_backward(lib, stream, f.data_ptr(), lin, gbar, _lib.ptr(g_next), out.data_ptr(), P, Cn, h, w, wrt, L._strides(out))
    return out


def gate(G, y):
    """G = y > 0 ? G : 0 in place over two dense f32 tensors of one shape, 16-byte aligned; returns G"""
    _check_f32("G", G, "a non-empty tensor", lambda t: t.numel() >= 1)
    _check_f32("y", y, f"{list(G.shape)}", lambda t: t.shape == G.shape)
    if G.numel() >= MAX_GATE:
        raise ValueError(f"G must hold fewer than 2^40 elements, got {G.numel()}")
    _check_gpu("G", G=G, y=y)
    if G.data_ptr() % 16 or y.data_ptr() % 16:
        raise ValueError("G and y must be 16-byte aligned")
    lib = entry()
    with _lib.on(G.device) as stream:
        _gate(lib, stream, G.data_ptr(), y.data_ptr(), G.numel())
    return G


class LpipsFunction(torch.autograd.Function):
    """value = net(img0, img1, normalize) with gradients in the images.  The forward keeps the thirteen post-ReLU maps; the backward
    consumes them, so it runs once."""

    @staticmethod
    def forward(ctx, img0, img1, net, normalize):
        value, state = net._forward_grad(img0, img1, normalize)
        ctx.net, ctx.state = net, state
        return value

    @staticmethod
    def backward(ctx, grad_value):
        if torch.is_grad_enabled():
            raise RuntimeError("LPIPSVGG: a double backward (create_graph=True) is not supported: the gradient in the images is computed "
                               "by HIP kernels that have no derivative of their own")
        if ctx.state is None:
            raise RuntimeError("LPIPSVGG: backward ran a second time for one forward; the stored activations were released by the first "
                               "(retain_graph=True does not keep them): call the net again")
        wrt = (WRT_FIRST if ctx.needs_input_grad[0] else 0) | (WRT_PARTNER if ctx.needs_input_grad[1] else 0)
        state, ctx.state = ctx.state, None
        if not wrt:
            return None, None, None, None
        d0, d1 = ctx.net._backward_grad(state, grad_value.reshape(-1).to(torch.float32).contiguous(), wrt)
        return d0, d1, None, None
