"""-m "not gpu": the backward of LPIPS-VGG without a GPU -- the float64 statement (tests/lpips_grad_ref.py) against torch's CPU float64
autograd, its tie and zero-norm rules on hand-built windows, the ctypes mirror of include/texgs_lpips_grad.h against gcc's layout,
the refusals that run before any launch or library call, and the autograd wiring of LPIPSVGG.__call__ with the chain stubbed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import lpips_grad_ref as GR  # noqa: E402
import lpips_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "texgs_lpips_grad.h")

# Both sides are float64 evaluations of one formula.  Measured worst |statement - autograd| / max|grad| over the cases below: 6.88e-15
# (profiles/lpips_grad_parity.json, "host_statement_vs_autograd"); the bound is 16 x that, rounded down, far inside the 1e-9 beyond
# which only a formula error can be the cause.
AUTOGRAD_BOUND = 16 * 6.8e-15
SMALL_WIDTHS = (16, 16, 32, 32, 48)


# ---- the statement against torch's autograd ----
def _torch_lpips(convs, lins, x, P, normalize):
    """The forward in torch CPU float64 ops, x [2P,3,H,W] -> the P values (differentiable)"""
    sc, sh = R.input_affine(normalize)
    h = x * torch.from_numpy(sc).double()[None, :, None, None] + torch.from_numpy(sh).double()[None, :, None, None]
    k, total = 0, 0.0
    for s, n in enumerate(R.SLICES):
        if s > 0:
            h = F.max_pool2d(h, 2)
        for _ in range(n):
            w, b = convs[k]
            h = F.conv2d(h, torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1).relu()
            k += 1
        f0, f1 = h[:P], h[P:]
        a = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        b_ = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((a - b_).pow(2) * torch.from_numpy(lins[s]).double()[None, :, None, None]).sum(1).mean((1, 2))
    return total


def statement_vs_autograd(size, seed=0):
    """One case -> (worst |statement - autograd|, max |autograd|, the statement's gradient)"""
    from texgs import lpips as L
    net = L.LPIPSVGG.random(11 + seed, widths=SMALL_WIDTHS)
    convs = [(w.numpy(), b.numpy()) for w, b in net.convs]
    lins = [l.numpy() for l in net.lins]
    H, W = size
    rng = np.random.default_rng(H * 100 + W + seed)
    P = 2
    img0 = rng.uniform(0, 1, (P, 3, H, W)).astype(np.float32)
    img1 = np.clip(img0 + rng.normal(0, 0.15, img0.shape), 0, 1).astype(np.float32)
    gbar = rng.uniform(0.5, 2.0, P)
    x = np.concatenate([img0, img1])
    maps = GR.forward_maps(convs, x, normalize=True)                     # masks from the statement's own forward
    for k in (1, 3, 6, 9, 12):                                           # no zero norm: torch's sqrt would return NaN there
        assert (np.sqrt((maps[k] ** 2).sum(1)) > 0).all()
    got = GR.backward(convs, lins, maps, gbar, normalize=True)
    xt = torch.from_numpy(x).double().requires_grad_()
    (_torch_lpips(convs, lins, xt, P, True) * torch.from_numpy(gbar)).sum().backward()
    want = xt.grad.numpy()
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(want).all()
    return float(np.abs(got - want).max()), float(np.abs(want).max()), got


@pytest.mark.parametrize("size", [(16, 16), (17, 31)], ids=["16x16", "17x31"])
def test_statement_agrees_with_torch_float64_autograd(size):
    diff, scale, got = statement_vs_autograd(size)
    print(f"statement vs autograd at {size}: {diff:.3e} of {scale:.3e} = {diff / scale:.3e} relative")
    assert scale > 0 and AUTOGRAD_BOUND <= 1e-9
    assert diff <= AUTOGRAD_BOUND * scale


def test_pieces_agree_with_torch_float64_autograd():
    rng = np.random.default_rng(5)
    # the transposed convolution: odd sizes, Cin != Cout, a batch
    g, w = rng.standard_normal((2, 16, 5, 7)), rng.standard_normal((16, 6, 3, 3))
    x = torch.zeros(2, 6, 5, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, torch.from_numpy(w), padding=1).backward(torch.from_numpy(g))
    got = GR.conv3x3_transposed(g, w)
    assert np.abs(got - x.grad.numpy()).max() <= 1e-13 * np.abs(got).max()
    assert GR.conv3x3_transposed(g, w, fp32=True).dtype == np.float32
    # and it is the forward convolution over the flipped, transposed weights
    wt = np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    assert np.abs(R.conv3x3(g, wt, np.zeros(6), relu=False) - got).max() <= 1e-13 * np.abs(got).max()
    # the unpool of an odd map: the last row and column get nothing
    f, gn = rng.standard_normal((2, 3, 7, 9)), rng.standard_normal((2, 3, 3, 4))
    t = torch.from_numpy(f).requires_grad_()
    F.max_pool2d(t, 2).backward(torch.from_numpy(gn))
    up = GR.unpool(f, gn)
    assert np.array_equal(up, t.grad.numpy()) and not up[..., 6, :].any() and not up[..., :, 8].any()
    # the head
    f0, f1 = np.abs(rng.standard_normal((2, 8, 3, 5))), np.abs(rng.standard_normal((2, 8, 3, 5)))
    f0[f0 < 0.3] = 0
    lin, gbar = rng.uniform(0, 1, 8), rng.uniform(0.5, 2, 2)
    a, b = torch.from_numpy(f0).requires_grad_(), torch.from_numpy(f1).requires_grad_()
    d = (a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10) - b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)).pow(2)
    ((d * torch.from_numpy(lin)[None, :, None, None]).sum(1).mean((1, 2)) * torch.from_numpy(gbar)).sum().backward()
    h0, h1 = GR.head_backward(f0, f1, lin, gbar)
    for got, want in ((h0, a.grad.numpy()), (h1, b.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    s0, s1 = GR.head_backward(f1, f0, lin, gbar)                          # swapping the images swaps the gradients, bit for bit
    assert np.array_equal(s0, h1) and np.array_equal(s1, h0)
    s0, s1 = GR.head_backward(f1, f0, lin, gbar, fp32=True)
    q0, q1 = GR.head_backward(f0, f1, lin, gbar, fp32=True)
    assert np.array_equal(s0, q1) and np.array_equal(s1, q0) and q0.dtype == np.float32 and 0 < np.abs(q0 - h0).max() < 1e-5 * np.abs(h0).max()


# ---- the two deliberate rules ----
def test_equal_maxima_send_the_gradient_to_the_first_in_row_major_order():
    f = np.zeros((1, 1, 2, 12))
    # windows: a single maximum in each position; two, three and four equal maxima; all zero
    f[0, 0, :, 0:2] = [[5, 1], [2, 3]]
    f[0, 0, :, 2:4] = [[1, 5], [2, 3]]
    f[0, 0, :, 4:6] = [[1, 2], [3, 5]]
    f[0, 0, :, 6:8] = [[1, 5], [5, 2]]              # two equal: the upper right one, row-major first
    f[0, 0, :, 8:10] = [[4, 4], [4, 4]]
    f[0, 0, :, 10:12] = 0.0
    assert GR.first_max(f)[0, 0, 0].tolist() == [0, 1, 3, 1, 0, 0]
    gn = np.arange(1.0, 7.0).reshape(1, 1, 1, 6)
    up = GR.unpool(f, gn)
    want = np.zeros((2, 12))
    want[0, 0], want[0, 3], want[1, 5], want[0, 7], want[0, 8], want[0, 10] = 1, 2, 3, 4, 5, 6
    assert np.array_equal(up[0, 0], want)
    # behind the gate the all-zero window receives nothing: its first maximum is a zero, and the ReLU is closed there
    G = GR.finish(f, np.ones_like(f), gn)
    assert G[0, 0, 0, 10] == 0 and not G[0, 0, :, 10:12].any() and G[0, 0, 0, 7] == 5 and G[0, 0, 1, 6] == 1
    assert GR.unpool(f.astype(np.float32), gn.astype(np.float32)).dtype == np.float32


def test_a_zero_norm_pixel_gets_a_zero_row_and_nothing_is_nan():
    rng = np.random.default_rng(8)
    f0, f1 = np.abs(rng.standard_normal((1, 4, 2, 2))), np.abs(rng.standard_normal((1, 4, 2, 2)))
    f0[0, :, 0, 1] = 0.0                              # a zero pixel in the first image
    f1[0, :, 1, 0] = 0.0                              # one in the partner
    f0[0, :, 1, 1] = 0.0
    f1[0, :, 1, 1] = 0.0                              # and one in both
    lin, gbar = rng.uniform(0.1, 1, 4), np.array([1.5])
    for fp32 in (False, True):
        h0, h1 = GR.head_backward(f0, f1, lin, gbar, fp32)
        assert np.isfinite(h0).all() and np.isfinite(h1).all()
        assert not h0[0, :, 0, 1].any() and not h1[0, :, 1, 0].any() and not h0[0, :, 1, 1].any() and not h1[0, :, 1, 1].any()
        assert h1[0, :, 0, 1].any() and h0[0, :, 1, 0].any() and h0[0, :, 0, 0].all()
    # against a zero partner and under equal lin weights the term is |a|^2 = 1 whatever f0 is: that row vanishes (up to the eps)
    h0, _ = GR.head_backward(f0, f1, lin * 0 + 1, gbar)
    assert np.abs(h0[0, :, 1, 0]).max() < 1e-9 < np.abs(h0[0, :, 0, 0]).max()


# ---- the C side without a GPU ----
def test_ctypes_mirror_matches_the_header(tmp_path):
    from texgs import lpips_grad as G
    consts = {"TEXGS_LPIPS_WRT_FIRST": G.WRT_FIRST, "TEXGS_LPIPS_WRT_PARTNER": G.WRT_PARTNER}
    assert abi_check.layout_mismatches("texgs_lpips_grad.h", G.MIRRORS, consts, tmp_path) == []
    body = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.findall(r"typedef struct (\w+) \{", body) == list(G.MIRRORS)


def test_every_prototype_has_a_signature_of_the_same_arity(lib_built):
    from texgs import _lib, lpips as L, lpips_grad as G
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(G.SIGNATURES) == ["texgs_lpips_gate", "texgs_lpips_head_backward"]
    assert abi_check.signature_mismatches(HDR, G.SIGNATURES, G.MIRRORS) == []
    lib = ctypes.CDLL(lib_built)
    for name in protos:
        assert hasattr(lib, name), name
    assert G.entry() is _lib.load() and lib_built == _lib.LIB_PATH
    assert G.entry().texgs_lpips_gate.argtypes == G.SIGNATURES["texgs_lpips_gate"][1]
    # a table of its own: disjoint from the main one and from the forward's, whose header keeps its five prototypes
    assert not set(G.SIGNATURES) & set(_lib.SIGNATURES) and not set(G.SIGNATURES) & set(L.SIGNATURES) and _lib.ABI_VERSION == 19
    assert len(abi_check.prototypes(os.path.join(ROOT, "include", "texgs_lpips.h"))) == 5 and not hasattr(L, "LpipsHeadBackwardStruct")


def test_entry_points_refuse_before_any_launch(lib_built):
    """Every refused argument returns an error that names it; nothing is launched (a launch here, without a GPU, would fail with a HIP
    error that does not name the argument)."""
    import ctypes as C
    from texgs import lpips as L, lpips_grad as G
    lib = G.entry()
    L.entry()
    err = lambda: lib.texgs_last_error().decode()
    buf = (C.c_float * 64)()              # stands in for every device pointer: a refused call reads none of them
    b = C.addressof(buf)

    def head(**kw):
        f = dict(f=b, lin=b, gbar=b, g_next=None, G=b, P=1, C=16, h=2, w=2, wrt=1)
        f.update(kw)
        return lib.texgs_lpips_head_backward(C.byref(G.LpipsHeadBackwardStruct(**f)), None)
    for kw, word in ((dict(P=0), "P must"), (dict(P=65536), "P must"), (dict(C=0), "C must"), (dict(C=513), "C must"), (dict(h=0), "h and w"),
                     (dict(w=0), "h and w"), (dict(h=1 << 16, w=1 << 15), "2^31"), (dict(wrt=0), "wrt"), (dict(wrt=4), "wrt"), (dict(wrt=-1), "wrt"),
                     (dict(f=None), "NULL"), (dict(lin=None), "NULL"), (dict(gbar=None), "NULL"), (dict(G=None), "NULL"),
                     (dict(g_next=b, h=1), "g_next"), (dict(g_next=b, w=1, h=4), "g_next"), (dict(f=b + 2), "4-byte"), (dict(g_next=b + 1), "4-byte"),
                     (dict(G=b + 3), "4-byte"), (dict(g_row=1, g_chan=4, g_img=64), "g_row"), (dict(g_row=2), "g_row"),
                     (dict(g_row=2, g_chan=3, g_img=64), "g_chan"), (dict(g_row=2, g_chan=4, g_img=63), "g_img"),
                     (dict(g_row=2, g_chan=4, g_img=-64), "g_img"), (dict(P=4, wrt=3, g_row=2, g_chan=4, g_img=1 << 60), "g_img")):
        assert L.entry().texgs_lpips_head_temp_bytes(0, 1, 1) == 0 and "P must" in err()          # another message first
        assert head(**kw) != 0, kw
        assert word in err(), (kw, err())
    assert lib.texgs_lpips_head_backward(None, None) != 0 and "NULL" in err()

    aligned = (b + 15) & ~15
    for args, word in (((aligned, aligned, 0), "n must"), ((aligned, aligned, -4), "n must"), ((aligned, aligned, 1 << 40), "n must"),
                       ((None, aligned, 8), "NULL"), ((aligned, None, 8), "NULL"), ((aligned + 4, aligned, 8), "16-byte"),
                       ((aligned, aligned + 8, 8), "16-byte")):
        assert L.entry().texgs_conv3x3_packed_bytes(0, 64, 0) == 0 and "Cin" in err()
        assert lib.texgs_lpips_gate(*args, None) != 0, args
        assert word in err(), (args, err())


def test_arguments_are_checked_before_the_library_is_loaded(monkeypatch):
    from texgs import _lib, lpips_grad as G
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_bound", {})             # no table counts as applied: entry() would have to load
    f, lin, gbar = torch.zeros(2, 16, 4, 6), torch.zeros(16), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.head_backward(f, lin, gbar, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.head_backward(f, lin, gbar, 3, g_next=torch.zeros(2, 16, 2, 3), out=torch.zeros(2, 16, 8, 10)[:, :, 2:6, 2:8])
    for wrt in (0, 4, None, "both"):
        with pytest.raises(ValueError, match="wrt must be"):
            G.head_backward(f, lin, gbar, wrt)
    with pytest.raises(ValueError, match=r"\[2P, C, h, w\]"):
        G.head_backward(torch.zeros(3, 16, 4, 6), lin, gbar, 1)
    with pytest.raises(ValueError, match="lin must be"):
        G.head_backward(f, torch.zeros(15), gbar, 1)
    with pytest.raises(ValueError, match="gbar must be"):
        G.head_backward(f, lin, torch.zeros(2), 1)
    with pytest.raises(ValueError, match="gbar must be torch.float32"):
        G.head_backward(f, lin, gbar.double(), 1)
    with pytest.raises(ValueError, match="g_next must be"):
        G.head_backward(f, lin, gbar, 1, g_next=torch.zeros(2, 16, 2, 3))        # wrt = 1 selects one image, not two
    with pytest.raises(ValueError, match="g_next must be"):
        G.head_backward(f, lin, gbar, 3, g_next=torch.zeros(2, 16, 4, 6))
    with pytest.raises(ValueError, match="at least 2x2"):
        G.head_backward(torch.zeros(2, 16, 1, 6), lin, gbar, 1, g_next=torch.zeros(1, 16, 0, 3))
    with pytest.raises(ValueError, match="out must be"):
        G.head_backward(f, lin, gbar, 1, out=torch.zeros(2, 16, 4, 6))
    with pytest.raises(ValueError, match="view"):
        G.head_backward(f, lin, gbar, 1, out=torch.zeros(1, 16, 4, 12)[:, :, :, ::2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.gate(torch.zeros(5), torch.zeros(5))
    with pytest.raises(ValueError, match="y must be"):
        G.gate(torch.zeros(5), torch.zeros(6))
    with pytest.raises(ValueError, match="G must be"):
        G.gate(torch.zeros(0), torch.zeros(0))
    with pytest.raises(ValueError, match="contiguous"):
        G.gate(torch.zeros(4, 4)[:, ::2], torch.zeros(4, 2))
    with pytest.raises(ValueError, match="float32"):
        G.gate(torch.zeros(4, dtype=torch.float64), torch.zeros(4))
    with pytest.raises(ValueError, match=r"\[Cout, Cin, 3, 3\]"):
        G.transposed_weight(torch.zeros(16, 3, 3))


def test_transposed_weight_flips_the_taps_and_pads_the_rows():
    from texgs import lpips as L, lpips_grad as G
    w = torch.arange(64 * 3 * 9, dtype=torch.float32).view(64, 3, 3, 3)
    t = G.transposed_weight(w)
    assert tuple(t.shape) == (16, 64, 3, 3) and t.is_contiguous() and not t[3:].any()
    assert t[2, 5, 0, 1] == w[5, 2, 2, 1] and t[0, 63, 2, 2] == w[63, 0, 0, 0]
    assert tuple(G.transposed_weight(torch.zeros(48, 24, 3, 3)).shape) == (32, 48, 3, 3)
    assert tuple(G.transposed_weight(torch.zeros(128, 64, 3, 3)).shape) == (64, 128, 3, 3)
    assert L.grad_activation_floats(1, 800, 800) == 345_600_000
    assert L.grad_activation_floats(2, 17, 31, (16, 16, 32, 32, 48)) == 4 * (2 * 16 * 17 * 31 + 2 * 16 * 8 * 15 + 3 * 32 * 4 * 7 + 3 * 32 * 2 * 3 + 3 * 48 * 1 * 1)


# ---- the autograd wiring, with the chain stubbed ----
class _Stub:
    """Stands in for LPIPSVGG._forward_grad / _backward_grad and records what reaches them"""

    def __init__(self, net):
        self.calls, self.net = [], net
        net._forward_grad = self.forward
        net._backward_grad = self.backward
        net.table = self.table

    def table(self, img0, img1, normalize=False, out=None):
        self.calls.append(("table", img0.requires_grad, img1.requires_grad))
        return torch.zeros(img0.shape[0] if img0.dim() == 4 else 1, 8, dtype=torch.float64)

    def forward(self, img0, img1, normalize):
        self.calls.append(("forward", bool(normalize)))
        P = img0.shape[0] if img0.dim() == 4 else 1
        return torch.full((P, 1, 1, 1), 0.25), dict(maps=[object()], shape=tuple(img0.shape))

    def backward(self, state, gbar, wrt):
        self.calls.append(("backward", wrt, tuple(gbar.shape), gbar.dtype, gbar.is_contiguous(), torch.is_grad_enabled()))
        assert state["maps"] is not None
        return (torch.full(state["shape"], 1.0) if wrt & 1 else None, torch.full(state["shape"], 2.0) if wrt & 2 else None)


def test_the_differentiable_path_is_taken_only_when_a_gradient_is_wanted():
    from texgs import lpips as L, metrics
    net = L.LPIPSVGG.random(2, widths=(16,) * 5)
    stub = _Stub(net)
    a, b = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    net(a, b)
    assert stub.calls == [("table", False, False)]
    a.requires_grad_()
    with torch.no_grad():
        net(a, b, normalize=True)
    assert stub.calls[-1][0] == "table" and len(stub.calls) == 2
    v = net(a, b, normalize=True)
    assert stub.calls[-1] == ("forward", True) and v.requires_grad and tuple(v.shape) == (2, 1, 1, 1)
    # the metric surfaces stay on the present path whatever the images require
    one = torch.rand(3, 16, 16, requires_grad=True)
    assert metrics.lpips(one, one.detach(), net=net) == 0.0
    assert stub.calls[-1][0] == "table"
    # ... and so do layers() and features(): they go through table() and _run(), which detach
    net.layers(a, b)
    assert stub.calls[-1][0] == "table"
    # img0 only: None for img1; the upstream gradient arrives as a dense f32 [P] with grad mode off
    (v.sum() * 3).backward()
    assert stub.calls[-1] == ("backward", 1, (2,), torch.float32, True, False)
    assert a.grad is not None and bool((a.grad == 1).all()) and b.grad is None
    # img1 only, unbatched
    c, d = torch.rand(3, 16, 16), torch.rand(3, 16, 16, requires_grad=True)
    net(c, d).backward()
    assert stub.calls[-1][:3] == ("backward", 2, (1,)) and c.grad is None and bool((d.grad == 2).all())
    # both
    e, f = torch.rand(1, 3, 16, 16, requires_grad=True), torch.rand(1, 3, 16, 16, requires_grad=True)
    net(e, f).mean().backward()
    assert stub.calls[-1][:2] == ("backward", 3) and bool((e.grad == 1).all()) and bool((f.grad == 2).all())


def test_second_and_double_backward_raise_by_name():
    from texgs import lpips as L
    net = L.LPIPSVGG.random(2, widths=(16,) * 5)
    stub = _Stub(net)
    a, b = torch.rand(1, 3, 16, 16, requires_grad=True), torch.rand(1, 3, 16, 16)
    v = net(a, b).sum()
    v.backward(retain_graph=True)
    n = len(stub.calls)
    with pytest.raises(RuntimeError, match="LPIPSVGG: backward ran a second time"):
        v.backward()
    assert len(stub.calls) == n                                          # the chain was not entered again
    v = net(a, b).sum()
    n = len(stub.calls)
    with pytest.raises(RuntimeError, match=r"LPIPSVGG: a double backward \(create_graph=True\)"):
        torch.autograd.grad(v, a, create_graph=True)
    assert len(stub.calls) == n
    v.backward()                                                         # the refused double backward released nothing
    assert stub.calls[-1][0] == "backward"


def test_the_dropin_inherits_the_differentiable_path(tmp_path):
    from texgs import lpips as L
    import lpips
    net = L.LPIPSVGG.random(5, widths=L.WIDTHS)
    torch.save({f"features.{i}.{leaf}": t for i, (w, b) in zip(L.VGG_INDICES, net.convs) for leaf, t in (("weight", w), ("bias", b))},
               tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}, tmp_path / "lin.pth")
    with pytest.warns(RuntimeWarning, match="UNPINNED"):
        m = lpips.LPIPS(net="vgg", model_path=str(tmp_path / "lin.pth"), vgg_path=str(tmp_path / "vgg16.pth"), verbose=False)
    stub = _Stub(m)
    a, b = torch.rand(1, 3, 16, 16, requires_grad=True), torch.rand(1, 3, 16, 16)
    m(a, b, normalize=True).sum().backward()
    assert [c[0] for c in stub.calls] == ["forward", "backward"] and stub.calls[0] == ("forward", True) and a.grad is not None
    m.forward(a.detach(), b)
    assert stub.calls[-1][0] == "table"
