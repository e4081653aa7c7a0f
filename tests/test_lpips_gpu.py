"""-m gpu: LPIPS-VGG in HIP (csrc/lpips.hip through texgs.lpips, texgs.metrics and the `lpips` drop-in) on the MI355X.

Every compared map t:   max|hip - f64| <= 4 x max( max|f32 - f64|, 2^-23 max|f64| )      (lpips_ref.tolerance)
f64 is tests/lpips_ref.py's float64 statement, f32 the same loops in float32 (a plain k-ordered fp32 chain): the 4x over another fp32
evaluation's own error is the margin of tests/test_mlp_gpu.py and tests/test_preprocess_gpu.py; the floor keeps an exactly representable
case from demanding zero.  ReLU and max-pool are continuous, so no element is excluded anywhere and there is no outlier budget.
For SCALARS (the layers' terms, the value) a single fp32 error can vanish by cancellation, so the maximum over all cases stands on both
sides of the same inequality: absolute for the whole-net cases, whose values have one scale; relative for the head-alone cases, whose
scale goes with 1/C (`_scalars_within`).

x and y of every convolution are views into NaN-filled buffers (tests/lpips_cases.py: NaN rows and columns around every channel
plane, a NaN plane between batch slots; the descriptor carries the strides): a tap read from outside an image surfaces as NaN, a
store outside y is seen in the guard cells afterwards.  One test runs the dense layout (strides 0) against the embedded one bit for
bit.  The cases are stated in tests/lpips_cases.py; edge sizes are derived from the tile constants texgs.lpips exports.
Only precision "fp32" exists: "bf16x3" is refused by name (tests/test_lpips_host.py), so it has no bound here.
Measured on one MI355X (scripts/lpips_parity.py -> profiles/lpips_parity.json): the worst ratio over all maps is 1.81 of the bound's 4;
the value at 32x48 (0.0065) is within 1.4e-10 of float64, far below the three decimals the metric is reported to."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_cases as K  # noqa: E402
import lpips_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _within(name, got, f64, f32):
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - f64).max())
    tol = R.tolerance(f64, f32)
    print(f"{name}: max|hip - f64| {err:.3e}, bound {tol:.3e}, ratio to the f32 statement's error (bound 4) {4 * err / tol:.2f}")
    assert err <= tol, (name, err, tol)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32 if t.dtype == torch.float32 else np.int64)


# ---- the convolution alone ----
def test_the_case_list_is_what_the_ids_say():
    assert len(K.conv_cases()) == K.N_CONV


@pytest.mark.parametrize("k", range(K.N_CONV))
def test_conv_matches_float64(k):
    c, d = K.conv_case(k)
    y = K.run_conv(c, d)
    assert not torch.isnan(y).any(), "a tap was read from outside x"
    _within(K.cid(c), y, d["y64"], d["y32"])
    if c["relu"]:
        assert float(y.min()) >= 0.0
    else:
        assert float(y.min()) < 0.0


def test_conv_image_has_the_same_bits_in_every_batch_slot():
    c, d = K.conv_case(5)                                                                 # 64 -> 64 at 9 x (2 TILE_W + 1)
    img = torch.from_numpy(np.array(d["x"][1:2])).cuda()
    other = torch.randn(1, *img.shape[1:], device="cuda")
    alone = K.run_conv(c, d, x=img.contiguous())
    in3 = K.run_conv(c, d, x=torch.cat([other, other * 2, img]).contiguous())
    in2 = K.run_conv(c, d, x=torch.cat([other, img]).contiguous())
    assert np.array_equal(_bits(alone[0]), _bits(in3[2])) and np.array_equal(_bits(alone[0]), _bits(in2[1]))
    assert not np.array_equal(_bits(alone[0]), _bits(in3[0]))


def test_conv_two_calls_and_a_side_stream_give_the_same_bits():
    c, d = K.conv_case(7)                                                                 # pool_in, two cout tiles
    first, second = K.run_conv(c, d), K.run_conv(c, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = K.run_conv(c, d)
    side.synchronize()
    assert np.array_equal(_bits(first), _bits(second)) and np.array_equal(_bits(first), _bits(third))


def test_conv_refused_arguments_launch_nothing():
    from texgs import lpips as L
    lib = L.entry()
    x = torch.randn(1, 16, 4, 4, device="cuda")
    bias = torch.randn(16, device="cuda")
    packed = L.pack_conv3x3(torch.randn(16, 16, 3, 3, device="cuda"))
    ybuf, y = K.embed((1, 16, 4, 4))
    good = dict(x=x.data_ptr(), packed=packed.data_ptr(), bias=bias.data_ptr(), in_scale=None, in_shift=None, y=y.data_ptr(), B=1, Cin=16,
                Cout=16, H=4, W=4, relu=1, pool_in=0, precision=0, y_row=y.stride(2), y_chan=y.stride(1), y_img=y.stride(0))
    stream = torch.cuda.current_stream().cuda_stream
    for kw, word in ((dict(Cout=24), "Cout"), (dict(Cin=513), "Cin"), (dict(packed=None), "packed"), (dict(precision=3), "precision"),
                     (dict(precision=1), "BF16X3"), (dict(H=1, pool_in=1), "pool_in"), (dict(in_scale=bias.data_ptr()), "in_scale"),
                     (dict(in_shift=bias.data_ptr()), "in_shift"), (dict(y_row=3), "y_row"), (dict(y_chan=4 * y.stride(2) - 1), "y_chan"),
                     (dict(x_row=4, x_chan=16, x_img=255), "x_img")):
        assert lib.texgs_conv3x3(C.byref(L.Conv3x3Struct(**dict(good, **kw))), stream) != 0, kw
        assert word in lib.texgs_last_error().decode(), (kw, lib.texgs_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all()), "a refused call wrote y"
    with pytest.raises(ValueError, match="Cout"):
        L.conv3x3(x, packed, torch.zeros(24, device="cuda"))
    with pytest.raises(ValueError, match="packed"):
        L.conv3x3(torch.randn(1, 8, 4, 4, device="cuda"), packed, bias)
    assert lib.texgs_conv3x3(C.byref(L.Conv3x3Struct(**good)), stream) == 0                # and the good call runs
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and K.guards_intact(ybuf, y)
    with pytest.raises(ValueError, match="view"):
        L.conv3x3(x[:, :, :, ::2], packed, bias)                                          # columns not adjacent


def test_conv_dense_and_embedded_layouts_give_the_same_bits():
    from texgs import lpips as L
    for k in (1, 7, 13):                                                                 # affine, pool_in, two images and two cout tiles
        c, d = K.conv_case(k)
        dense = L.conv3x3(K.cuda(d["x"]), L.pack_conv3x3(K.cuda(d["w"])), K.cuda(d["b"]), relu=c["relu"], pool_in=c["pool"],
                          in_scale=K.cuda(d["sc"]), in_shift=K.cuda(d["sh"]))
        assert dense.is_contiguous() and np.array_equal(_bits(dense), _bits(K.run_conv(c, d).contiguous())), k


# ---- the head alone ----
def _scalars_within(name, got, f64, f32, relative):
    """max over all scalars of the hip error <= 4 x max(max over all scalars of the f32 statement's error, 2^-23 of the scale)"""
    got, f64, f32 = (np.asarray(a, np.float64).reshape(-1) for a in (got, f64, f32))
    scale = np.abs(f64) if relative else np.full_like(f64, np.abs(f64).max())
    assert (scale > 0).all()
    err, yard = (np.abs(got - f64) / scale).max(), (np.abs(f32 - f64) / scale).max()
    print(f"{name}: max hip error {err:.3e}, max f32-statement error {yard:.3e} ({'relative' if relative else 'of the largest value'}), "
          f"ratio (bound 4) {err / max(yard, 2.0 ** -23):.2f}")
    assert err <= 4.0 * max(yard, 2.0 ** -23), (name, err, yard)


def test_head_matches_float64():
    from texgs import lpips as L
    got, v64, v32 = [], [], []
    for k, (P, Cn, h, w, special) in enumerate(K.HEAD_CASES):
        d = K.head_case(k)
        t = K.run_head(K.cuda(d["f"]), K.cuda(d["lin"]), layer=k % 4)
        col = t[:, k % 4].cpu().numpy()
        assert np.isfinite(col).all() and (col > 0).all(), (k, col)
        others = [j for j in range(L.ROW) if j != k % 4]
        assert bool(torch.isnan(t[:, others]).all()), "the head wrote another column"
        got.append(col); v64.append(d["v64"]); v32.append(d["v32"])
    _scalars_within("head", np.concatenate(got), np.concatenate(v64), np.concatenate(v32), relative=True)


def test_head_layer_4_writes_the_sum_and_leaves_the_reserved_columns():
    from texgs import lpips as L
    d = K.head_case(1)
    f, lin = K.cuda(d["f"]), K.cuda(d["lin"])
    t = torch.full((3, L.ROW), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :4] = torch.tensor([[0.5, 0.25, 0.125, 1.0]], dtype=torch.float64)
    K.run_head(f, lin, layer=4, table=t)
    h = t.cpu().numpy()
    assert np.array_equal(h[:, 5], (((h[:, 0] + h[:, 1]) + h[:, 2]) + h[:, 3]) + h[:, 4]) and np.isnan(h[:, 6:]).all()
    assert np.array_equal(h[:, 4], K.run_head(f, lin, layer=0).cpu().numpy()[:, 0])


def test_head_swap_and_two_calls_give_the_same_bits():
    for k in (2, 4, 5, 6):
        d = K.head_case(k)
        P = K.HEAD_CASES[k][0]
        f, lin = K.cuda(d["f"]), K.cuda(d["lin"])
        a, b = K.run_head(f, lin), K.run_head(f, lin)
        s = K.run_head(torch.cat([f[P:], f[:P]]).contiguous(), lin)
        assert np.array_equal(_bits(a[:, 0]), _bits(b[:, 0])) and np.array_equal(_bits(a[:, 0]), _bits(s[:, 0])), k
    z = torch.zeros(2, 64, 3, 5, device="cuda")
    assert float(K.run_head(z, K.cuda(K.head_case(1)["lin"]))[0, 0]) == 0.0                   # 0 / (0 + 1e-10) = 0, never NaN


# ---- the whole net ----
@pytest.mark.parametrize("size", K.NET_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_net_features_match_float64(size):
    net, _, _ = K.net()
    d = K.net_case(size)
    x = K.cuda(np.concatenate([d["img0"], d["img1"]]))
    taps = net.features(x, normalize=True)
    assert [tuple(t.shape) for t in taps] == [tuple(t.shape) for t in d["taps64"]]
    for k, t in enumerate(taps):
        _within(f"{size} relu{k + 1}", t, d["taps64"][k], d["taps32"][k])
    one = net.features(x[2], normalize=True)                                             # unbatched: the same bits as in the batch
    assert all(np.array_equal(_bits(a[0]), _bits(b[2])) for a, b in zip(one, taps))


def test_net_layers_and_value_match_float64():
    """The scalars of all whole-net cases (three sizes, P = 1 and P = 2) stand together on both sides of the inequality"""
    net, _, _ = K.net()
    got_l, l64, l32, got_v = [], [], [], []
    for size in K.NET_SIZES:
        d = K.net_case(size)
        a, b = K.cuda(d["img0"]), K.cuda(d["img1"])
        both = net.layers(a, b, normalize=True)
        alone = net.layers(a[0], b[0], normalize=True)
        assert tuple(both.shape) == (2, 5) and tuple(alone.shape) == (1, 5) and both.dtype == torch.float64
        assert np.array_equal(_bits(alone[0]), _bits(both[0])), "a pair alone and inside P = 2 differ"
        value = net(a, b, normalize=True)
        assert tuple(value.shape) == (2, 1, 1, 1) and value.dtype == torch.float32 and value.is_cuda
        assert tuple(net(a[0], b[0], normalize=True).shape) == (1, 1, 1, 1)
        assert np.array_equal(_bits(net(a[1], b[1], normalize=True)).ravel(), _bits(value[1]).ravel())
        got_l.append(both.cpu().numpy()); l64.append(d["layers64"]); l32.append(d["layers32"]); got_v.append(value.cpu().numpy().reshape(-1))
        print(f"{size}: LPIPS {value.reshape(-1).tolist()}, |hip - f64| {np.abs(got_v[-1] - K.value(d['layers64'])).tolist()}")
    got_l, l64, l32 = np.concatenate(got_l), np.concatenate(l64), np.concatenate(l32)
    for k in range(5):
        _scalars_within(f"layer {k}", got_l[:, k], l64[:, k], l32[:, k], relative=False)
    v64, v32 = K.value(l64), K.value(l32)
    err, yard = np.abs(np.concatenate(got_v) - v64).max(), np.abs(v32 - v64).max()
    # the value is returned as float32: its own rounding (2^-24 relative) joins the yardstick
    assert err <= 4.0 * max(yard, 2.0 ** -23 * np.abs(v64).max()), (err, yard)


def test_net_identical_pair_swap_and_zero_features():
    from texgs import lpips as L
    net, _, _ = K.net()
    d = K.net_case((17, 31))
    a, b = K.cuda(d["img0"]), K.cuda(d["img1"])
    assert net(a, a.clone(), normalize=True).reshape(-1).tolist() == [0.0, 0.0]
    assert float(net.layers(a[0], a[0].clone()).abs().max()) == 0.0
    ab, ba = net.table(a, b, normalize=True), net.table(b, a, normalize=True)
    assert np.array_equal(_bits(ab[:, :6]), _bits(ba[:, :6])) and float(ab[:, 5].min()) > 0.0
    assert bool((ab[:, 6:] == 0).all())                                                   # the reserved columns keep the caller's zeros
    assert np.array_equal(_bits(net(a, b)), _bits(net(a, b))) and not np.array_equal(_bits(net(a, b)), _bits(net(a, b, normalize=True)))
    # a first convolution whose bias of -1e3 leaves every feature of both images equal (relu1_1 == 0): exactly 0.0
    vgg = {f"features.{i}.{leaf}": t.clone() for i, (w, bb) in zip(L.VGG_INDICES, net.convs) for leaf, t in (("weight", w), ("bias", bb))}
    vgg["features.0.bias"].fill_(-1e3)
    lin = {f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}
    dead = L.LPIPSVGG(vgg, lin, _warn=False)
    t = dead.features(a, normalize=True)[0]
    assert torch.equal(t.amax((2, 3)), t.amin((2, 3)))                                   # relu1_2 = relu(bias) at every pixel, the border included
    assert dead(a, b, normalize=True).reshape(-1).tolist() == [0.0, 0.0]


def test_metrics_lpips_and_evaluator_column():
    from texgs import metrics
    net, _, _ = K.net()
    d = K.net_case((17, 31))
    views = [(K.cuda((d["img0"][k % 2] * 1.2 - 0.1 + 0.01 * k).astype(np.float32)), K.cuda(d["img1"][k % 2])) for k in range(3)]      # outside [0,1]: clamped
    want = [net(a.clamp(0, 1), b.clamp(0, 1), normalize=True) for a, b in views]
    v = metrics.lpips(views[0][0].clamp(0, 1), views[0][1], net=net)
    assert isinstance(v, float) and v == float(want[0].item())
    metrics.set_lpips(net)
    try:
        assert metrics.lpips(views[0][0].clamp(0, 1), views[0][1]) == v
    finally:
        metrics.set_lpips(None)
    plain, with_net = metrics.Evaluator(3), metrics.Evaluator(4, lpips=net)
    for a, b in views:
        plain.add(a, b)
        with_net.add(a, b)
    r0, r1 = plain.result(), with_net.result()
    assert list(r1) == list(r0) + ["lpips", "avg_error"]
    assert all(r0[k] == r1[k] for k in r0), (r0, r1)                                     # l1 / psnr / ssim unchanged bit for bit
    assert np.array_equal(_bits(plain.rows()), _bits(with_net.rows()))
    mean = float(np.mean([float(t.double().item()) for t in want]))
    assert abs(r1["lpips"] - mean) <= 2.0 ** -23 * mean                                  # (the table holds float64, net() returns float32)
    assert r1["avg_error"] == metrics.avg_error(r1["psnr"], r1["ssim"], r1["lpips"])
    unclamped = metrics.Evaluator(1, lpips=net)
    unclamped.add(*views[0], clamp=False)
    assert unclamped.result()["lpips"] != with_net._lpips_table[0, 5].item()


def test_dropin_returns_the_bits_of_lpipsvgg(tmp_path):
    from texgs import lpips as L
    import lpips
    net, _, _ = K.net()
    torch.save({f"net.slice{s}.{i}.{leaf}": t for i, s, (w, b) in zip(L.VGG_INDICES, L.SLICE_OF_INDEX, net.convs)
                for leaf, t in (("weight", w), ("bias", b))}, tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}, tmp_path / "vgg.pth")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        m = lpips.LPIPS(net="vgg", model_path=str(tmp_path / "vgg.pth"), vgg_path=str(tmp_path / "vgg16.pth")).to("cuda")
    d = K.net_case((16, 16))
    a, b = K.cuda(d["img0"][0]), K.cuda(d["img1"][0])
    got = m(a, b, normalize=True)
    assert tuple(got.shape) == (1, 1, 1, 1) and isinstance(got.item(), float)
    assert np.array_equal(_bits(got), _bits(net(a, b, normalize=True)))
