"""The cases of the LPIPS backward's GPU checks, stated once: tests/test_lpips_grad_gpu.py asserts on them and
scripts/lpips_grad_parity.py measures them.  Inputs by seed, both CPU evaluations of tests/lpips_grad_ref.py (float64 and the same
loops in float32) computed once per case and shared read-only, and the helpers that run a case on the GPU.

Every kernel output is a VIEW into a NaN-filled buffer (lpips_cases.embed, or a 1-D buffer with NaN on both sides for the gate), and the
guard cells are looked at after every call.  Each `measure_*` returns (worst |hip - f64|, the yardstick): the yardstick is
max(max |f32 - f64|, 2^-23 max |f64|) of the compared map, and the stage's bound is 4 of it (lpips_ref.tolerance)."""
import functools

import numpy as np
import torch

import lpips_cases as C
import lpips_grad_ref as GR

BOUND = 4.0


def yardstick(f64, f32):
    f64 = np.asarray(f64, np.float64)
    return max(float(np.abs(np.asarray(f32, np.float64) - f64).max()), 2.0 ** -23 * float(np.abs(f64).max()))


def err(hip, f64):
    hip = hip.detach().cpu().numpy() if torch.is_tensor(hip) else hip
    assert np.isfinite(hip).all(), "the kernel's output holds a NaN or an infinity"
    return float(np.abs(hip.astype(np.float64) - f64).max())


def _freeze(d):
    for v in d.values():
        for a in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return d


# ---- the head's backward alone ----
# (index into lpips_cases.HEAD_CASES, with g_next, planted): every shape without g_next; with it, every shape of at least 2x2
HEAD_BWD_CASES = [(k, False, False) for k in range(len(C.HEAD_CASES))] \
    + [(k, True, False) for k, c in enumerate(C.HEAD_CASES) if c[2] >= 2 and c[3] >= 2] + [(4, True, True)]


def head_id(case):
    k, with_next, planted = case
    P, Cn, h, w, special = C.HEAD_CASES[k]
    return f"{P}x{Cn}x{h}x{w}" + (f"-{special}" if special else "") + ("-gnext" if with_next else "") + ("-planted" if planted else "")


@functools.lru_cache(maxsize=None)
def head_bwd_case(i):
    k, with_next, planted = HEAD_BWD_CASES[i]
    P, Cn, h, w, _ = C.HEAD_CASES[k]
    d = C.head_case(k)
    f, lin = np.array(d["f"]), d["lin"]
    rng = np.random.default_rng(700 + i)
    if planted:                                             # 37x41 over 18x20: the last row and column belong to no window
        f[:, :, 4:6, 6:8] = 7.0                             # four equal maxima: the first takes the gradient
        f[:, :, 10, 13] = f[:, :, 11, 12] = 9.0             # two equal maxima on the anti-diagonal: the upper right one
        f[:, :, 11, 15] = f[:, :, 11, 14] = 8.0             # two in the lower row: the left one
        f[:, :, 20:24, 20:26] = 0.0                         # all-zero windows: the first cell, behind a closed gate
    gbar = rng.uniform(0.5, 2.0, P).astype(np.float32)
    g_next = rng.standard_normal((2 * P, Cn, h // 2, w // 2)).astype(np.float32) if with_next else None
    out = dict(f=f, lin=lin, gbar=gbar, g_next=g_next)
    for tag, fp32 in (("64", False), ("32", True)):
        h0, h1 = GR.head_backward(f[:P], f[P:], lin, gbar, fp32)
        out["G" + tag] = GR.finish(f, np.concatenate([h0, h1]), g_next, fp32)
    return _freeze(out)


def run_head_backward(d, wrt):
    """One case on the GPU for one `wrt`: G is a view into a NaN-filled [2P, ...] buffer, of which only the selected half is handed
    to the call -> (the selected slots of G, a slice of the 2P)"""
    from texgs import lpips_grad as G
    P = d["f"].shape[0] // 2
    buf, view = C.embed(d["f"].shape)
    sel = {1: slice(0, P), 2: slice(P, 2 * P), 3: slice(0, 2 * P)}[wrt]
    g_next = None if d["g_next"] is None else C.cuda(d["g_next"][sel])
    got = G.head_backward(C.cuda(d["f"]), C.cuda(d["lin"]), C.cuda(d["gbar"]), wrt, g_next=g_next, out=view[sel])
    torch.cuda.synchronize()
    assert got.data_ptr() == view[sel].data_ptr()
    assert C.guards_intact(buf, view), "the kernel wrote outside G"
    rest = torch.ones(2 * P, dtype=torch.bool)
    rest[sel] = False
    assert bool(torch.isnan(view[rest.cuda()]).all()), "a slot that wrt does not select was written"
    return view[sel], sel


def measure_head_backward(i, wrt):
    d = head_bwd_case(i)
    got, sel = run_head_backward(d, wrt)
    return err(got, d["G64"][sel]), yardstick(d["G64"][sel], d["G32"][sel])


# ---- the gate ----
GATE_COUNTS = [1, 3, 5 * 37, 2 * 1024 + 1, 4096 * 1024 + 1024 + 3]       # the last: past one sweep of the grid, with a tail
GATE_GUARD = 16                                                         # NaN floats on both sides (64 bytes: the view stays aligned)


def gate_case(n):
    rng = np.random.default_rng(900 + n % 1000)
    y = np.maximum(rng.standard_normal(n), 0).astype(np.float32)         # a post-ReLU map: exact zeros ...
    y[rng.integers(0, n, max(1, n // 7))] = -0.0                          # ... negative zeros ...
    if n > 4:
        y[-2] = -1.0                                                      # ... and, against the contract, a negative: the gate is closed
    y[-1] = 0.5 if n > 1 else -0.0
    g = rng.standard_normal(n).astype(np.float32)
    g[y <= 0] = np.where(rng.uniform(size=int((y <= 0).sum())) < 0.5, np.nan, np.inf)      # a closed gate stores 0 whatever G held
    return g, y, np.where(y > 0, g, np.float32(0))


def run_gate(g, y):
    from texgs import lpips_grad as G
    n = g.shape[0]
    buf = torch.full((n + 2 * GATE_GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[GATE_GUARD:GATE_GUARD + n]
    view.copy_(torch.from_numpy(g))
    yt = torch.from_numpy(y).cuda()
    y_before = yt.clone()
    assert G.gate(view, yt) is view
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GATE_GUARD]).all()) and bool(torch.isnan(buf[GATE_GUARD + n:]).all()), "the kernel wrote outside G"
    assert torch.equal(yt.view(torch.int32), y_before.view(torch.int32)), "y was written"
    return view


# ---- the transposed weights through conv3x3 ----
# the FORWARD convolution (Cin -> Cout over B x H x W) whose data gradient is taken
CONVT_CASES = [(3, 64, 1, 16, 16), (3, 64, 2, 17, 23), (24, 48, 2, 5, 37), (64, 128, 1, 19, 21), (512, 512, 1, 3, 3)]


@functools.lru_cache(maxsize=None)
def convt_case(i):
    Cin, Cout, B, H, W = CONVT_CASES[i]
    rng = np.random.default_rng(500 + i)
    g = rng.standard_normal((B, Cout, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    return _freeze(dict(g=g, w=w, d64=GR.conv3x3_transposed(g, w), d32=GR.conv3x3_transposed(g, w, fp32=True)))


def run_convt(i):
    """-> (the data gradient [B, Cin, H, W], the padded channels behind it)"""
    from texgs import lpips as L, lpips_grad as G
    Cin, Cout, B, H, W = CONVT_CASES[i]
    d = convt_case(i)
    wt = G.transposed_weight(torch.from_numpy(np.array(d["w"]))).cuda()
    _, gv = C.embed(d["g"])
    ybuf, yv = C.embed((B, wt.shape[0], H, W))
    L.conv3x3(gv, L.pack_conv3x3(wt), torch.zeros(wt.shape[0], device="cuda"), relu=False, out=yv)
    torch.cuda.synchronize()
    assert C.guards_intact(ybuf, yv), "the kernel wrote outside y"
    return yv[:, :Cin], yv[:, Cin:]


def measure_convt(i):
    d = convt_case(i)
    got, pad = run_convt(i)
    assert not bool(pad.any()), "a padded channel of the data gradient is not zero"
    return err(got, d["d64"]), yardstick(d["d64"], d["d32"])


# ---- the whole chain ----
CHAIN_SIZES = [(16, 16), (17, 31), (32, 48), (24, 70)]


def chain_inputs(size):
    H, W = size
    rng = np.random.default_rng(H * 100 + W)
    img0 = rng.uniform(0, 1, (2, 3, H, W)).astype(np.float32)
    img1 = np.clip(img0 + rng.normal(0, 0.15, img0.shape), 0, 1).astype(np.float32)
    gbar = rng.uniform(0.5, 2.0, 2).astype(np.float32)
    return img0, img1, gbar


@functools.lru_cache(maxsize=None)
def chain_case(size):
    """The GPU forward's own thirteen maps, read back, and both CPU evaluations of the backward GIVEN those maps"""
    net, convs, lins = C.net()
    img0, img1, gbar = chain_inputs(size)
    _, state = net._forward_grad(C.cuda(img0), C.cuda(img1), True)
    maps = [m.cpu().numpy() for m in state["maps"]]
    out = dict(img0=img0, img1=img1, gbar=gbar, maps=maps)
    for tag, fp32 in (("64", False), ("32", True)):
        out["d" + tag] = GR.backward(convs, lins, maps, gbar, normalize=True, fp32=fp32)
    return _freeze(out)


def run_chain(size, wrt):
    """A fresh forward and the backward for `wrt` -> (d img0, d img1), None for the one left out"""
    net, _, _ = C.net()
    d = chain_case(size)
    _, state = net._forward_grad(C.cuda(d["img0"]), C.cuda(d["img1"]), True)
    out = net._backward_grad(state, C.cuda(d["gbar"]), wrt)
    torch.cuda.synchronize()
    return out


def measure_chain(size, wrt):
    """-> [(which, err, yardstick)] for the gradients that `wrt` selects"""
    d = chain_case(size)
    d0, d1 = run_chain(size, wrt)
    assert (d0 is None) == (not wrt & 1) and (d1 is None) == (not wrt & 2)
    rows = []
    for which, got, sel in (("img0", d0, slice(0, 2)), ("img1", d1, slice(2, 4))):
        if got is not None:
            assert tuple(got.shape) == d["img0"].shape and got.dtype == torch.float32
            rows.append((which, err(got, d["d64"][sel]), yardstick(d["d64"][sel], d["d32"][sel])))
    return rows
