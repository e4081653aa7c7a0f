"""-m "not gpu": the LPIPS stage without a GPU -- the float64 statement (tests/lpips_ref.py) against torch's CPU float64 chain, the
weight loading of texgs.lpips, the `lpips` drop-in's refusals, the argument checks that run before any library call, the entry points'
refusals that run before any launch, the ctypes mirrors of include/texgs_lpips.h against gcc's layout, and texgs.metrics.Evaluator's
unchanged result without a net."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import lpips_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "texgs_lpips.h")


# ---- the statement ----
@pytest.mark.parametrize("case", [dict(B=2, Cin=5, Cout=16, H=6, W=7, pool=False, affine=False, relu=True),
                                  dict(B=1, Cin=4, Cout=16, H=9, W=11, pool=True, affine=False, relu=True),     # odd size under the pool
                                  dict(B=2, Cin=3, Cout=32, H=5, W=8, pool=False, affine=True, relu=False)],
                         ids=["plain", "pool-odd", "affine"])
def test_statement_agrees_with_torch_float64(case):
    """A second implementation pins the statement: torch's CPU float64 conv2d / max_pool2d, within 1e-12 relative"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((case["B"], case["Cin"], case["H"], case["W"])).astype(np.float32)
    w = rng.standard_normal((case["Cout"], case["Cin"], 3, 3)).astype(np.float32)
    b = rng.standard_normal(case["Cout"]).astype(np.float32)
    sc = sh = None
    if case["affine"]:
        sc, sh = rng.uniform(0.5, 2.0, case["Cin"]).astype(np.float32), rng.uniform(0.5, 1.5, case["Cin"]).astype(np.float32)
    got = R.conv3x3(x, w, b, case["relu"], case["pool"], sc, sh)
    t = torch.from_numpy(x).double()
    if case["affine"]:
        t = t * torch.from_numpy(sc).double()[None, :, None, None] + torch.from_numpy(sh).double()[None, :, None, None]
    if case["pool"]:
        t = F.max_pool2d(t, 2)
    want = F.conv2d(t, torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)
    if case["relu"]:
        want = want.relu()
    want = want.numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    got32 = R.conv3x3(x, w, b, case["relu"], case["pool"], sc, sh, fp32=True)
    assert got32.dtype == np.float32 and 0 < np.abs(got32 - want).max() <= 1e-4 * np.abs(want).max()


def _small_net(seed, widths=(16, 16, 32, 32, 32)):
    from texgs import lpips as L
    net = L.LPIPSVGG.random(seed, widths=widths)
    convs = [(w.numpy(), b.numpy()) for w, b in net.convs]
    lins = [l.numpy() for l in net.lins]
    return net, convs, lins


def test_statement_identical_pair_and_zero_features():
    _, convs, lins = _small_net(1)
    rng = np.random.default_rng(4)
    a = rng.uniform(0, 1, (2, 3, 16, 19)).astype(np.float32)
    for fp32 in (False, True):
        assert (R.lpips(convs, lins, a, a.copy(), normalize=True, fp32=fp32) == 0.0).all()
    b = rng.uniform(0, 1, (2, 3, 16, 19)).astype(np.float32)
    v = R.lpips(convs, lins, a, b, normalize=True)
    assert (v > 0).all() and np.isfinite(v).all()
    z = np.zeros((1, 16, 3, 4))
    f = rng.standard_normal((1, 16, 3, 4))
    assert R.head(z, z, lins[0]) == 0.0                                   # 0 / (0 + 1e-10) = 0, never NaN
    one = R.head(z, f, lins[0])
    assert np.isfinite(one).all() and one > 0
    f[:, :, 1, 2] = 0.0                                                   # a single all-zero pixel
    assert np.isfinite(R.head(f, f * 0.5, lins[0])).all()


# ---- the weights ----
def test_both_weight_namings_load_the_same_tensors():
    from texgs import lpips as L
    net = L.LPIPSVGG.random(7)
    tv = {f"features.{i}.{leaf}": t for i, (w, b) in zip(L.VGG_INDICES, net.convs) for leaf, t in (("weight", w), ("bias", b))}
    pk = {f"net.slice{s}.{i}.{leaf}": t for i, s, (w, b) in zip(L.VGG_INDICES, L.SLICE_OF_INDEX, net.convs)
          for leaf, t in (("weight", w), ("bias", b))}
    lin_a = {f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}
    lin_b = {f"lins.{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}
    with pytest.warns(RuntimeWarning, match="UNPINNED") as rec:
        a = L.LPIPSVGG(tv, lin_a)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1          # the unpinned warning fires once
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        b = L.LPIPSVGG(pk, lin_b)
    assert len(a.convs) == len(b.convs) == 13 and len(a.lins) == len(b.lins) == 5
    for (w0, b0), (w1, b1), (w2, b2) in zip(a.convs, b.convs, net.convs):
        assert torch.equal(w0, w1) and torch.equal(b0, b1) and torch.equal(w0, w2) and torch.equal(b0, b2)
    for l0, l1, c in zip(a.lins, b.lins, L.WIDTHS):
        assert torch.equal(l0, l1) and tuple(l0.shape) == (c,)
    assert [tuple(w.shape) for w, _ in a.convs][:3] == [(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3)]


def test_missing_and_misshaped_keys_raise_by_name(tmp_path):
    from texgs import lpips as L
    net = L.LPIPSVGG.random(7, widths=(16, 16, 16, 16, 16))
    good_v = {f"features.{i}.{leaf}": t for i, (w, b) in zip(L.VGG_INDICES, net.convs) for leaf, t in (("weight", w), ("bias", b))}
    good_l = {f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}
    mk = lambda v, l: L.LPIPSVGG(v, l, widths=(16,) * 5, _warn=False)
    mk(good_v, good_l)
    v = dict(good_v); del v["features.12.bias"]
    with pytest.raises(KeyError, match=r"features\.12\.bias.*net\.slice3\.12\.bias"):
        mk(v, good_l)
    v = dict(good_v); v["features.5.weight"] = torch.zeros(16, 16, 3, 2)
    with pytest.raises(ValueError, match=r"features\.5\.weight.*\(16, 16, 3, 3\)"):
        mk(v, good_l)
    l = dict(good_l); del l["lin3.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        mk(good_v, l)
    l = dict(good_l); l["lin0.model.1.weight"] = torch.zeros(16)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight.*\(1, 16, 1, 1\)"):
        mk(good_v, l)
    # paths are loaded with weights_only=True
    pv, pl = tmp_path / "v.pth", tmp_path / "l.pth"
    torch.save(good_v, pv); torch.save(good_l, pl)
    from_files = mk(str(pv), pl)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(from_files.convs, net.convs))
    with pytest.raises(NotImplementedError, match="bf16x3"):
        L.LPIPSVGG.random(1, precision="bf16x3")
    with pytest.raises(ValueError, match="precision"):
        L.LPIPSVGG.random(1, precision="fp16")


def test_random_weights_are_seeded_and_lin_is_non_negative():
    from texgs import lpips as L
    a, b, c = L.LPIPSVGG.random(3), L.LPIPSVGG.random(3), L.LPIPSVGG.random(4)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a.convs, b.convs)) and not torch.equal(a.convs[0][0], c.convs[0][0])
    assert all((l >= 0).all() for l in a.lins)
    assert (L.TILE_H, L.TILE_W, L.K_STEP, L.COUT_TILE, L.CIN_STEP) == (8, 32, 72, 64, 8) and L.K_STEP == 9 * L.CIN_STEP


def test_activation_buffers_hold_the_largest_map_of_any_width_tuple():
    """The two ping-pong buffers are sized by the largest map a convolution writes, not by slice 0's: a width tuple that grows faster
    than the pools shrink the map (16 -> 128 channels at a quarter of the pixels) needs more than B x widths[0] x H x W floats."""
    from texgs import lpips as L
    assert L.activation_floats(2, 800, 800) == 2 * 64 * 800 * 800                        # VGG16: slice 0 is the largest
    assert L.activation_floats(2, 1200, 1600) * 4 / 1e9 == pytest.approx(0.98, abs=0.01)
    for B, H, W, widths in ((2, 16, 16, (16, 128, 128, 128, 128)), (1, 17, 31, (16, 16, 512, 16, 16)), (4, 33, 47, (16, 32, 64, 512, 512)),
                            (2, 32, 48, L.WIDTHS)):
        need, h, w = L.activation_floats(B, H, W, widths), H, W
        for s, c in enumerate(widths):
            if s:
                h, w = h // 2, w // 2
            assert need >= B * c * h * w, (widths, s)                                    # every slice's output fits
    assert L.activation_floats(2, 16, 16, (16, 128, 128, 128, 128)) == 2 * 128 * 8 * 8 > 2 * 16 * 16 * 16
    assert L.activation_floats(1, 17, 31, (16, 16, 512, 16, 16)) == 512 * 4 * 7


# ---- the drop-in ----
def test_dropin_refuses_by_name_and_never_downloads(tmp_path, monkeypatch):
    monkeypatch.setenv("TEXGS_LPIPS_LIN", str(tmp_path / "nothing" / "vgg.pth"))
    monkeypatch.setenv("TEXGS_LPIPS_VGG", str(tmp_path / "nothing" / "vgg16-397923af.pth"))
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    import lpips
    assert lpips.__file__.startswith(os.path.join(ROOT, "texture-gs_amd"))
    with pytest.raises(FileNotFoundError) as e:
        lpips.LPIPS(net="vgg")
    for word in ("vgg.pth", "vgg16-397923af.pth", "TEXGS_LPIPS_LIN", "TEXGS_LPIPS_VGG"):
        assert word in str(e.value)
    monkeypatch.delenv("TEXGS_LPIPS_LIN"); monkeypatch.delenv("TEXGS_LPIPS_VGG")
    with pytest.raises(FileNotFoundError, match="TEXGS_LPIPS_LIN"):
        lpips.LPIPS(net="vgg")
    with pytest.raises(NotImplementedError, match="alex"):
        lpips.LPIPS(net="alex")
    with pytest.raises(NotImplementedError, match="alex"):
        lpips.LPIPS()                                       # the package's default net
    with pytest.raises(NotImplementedError, match="squeeze"):
        lpips.LPIPS(net="squeeze")
    with pytest.raises(NotImplementedError, match="spatial=True"):
        lpips.LPIPS(net="vgg", spatial=True)
    with pytest.raises(NotImplementedError, match="lpips=False"):
        lpips.LPIPS(net="vgg", lpips=False)
    with pytest.raises(NotImplementedError, match="pretrained=False"):
        lpips.LPIPS(net="vgg", pretrained=False)


def test_dropin_loads_two_files_and_returns_self(tmp_path):
    from texgs import lpips as L
    import lpips
    net = L.LPIPSVGG.random(5)
    torch.save({f"features.{i}.{leaf}": t for i, (w, b) in zip(L.VGG_INDICES, net.convs) for leaf, t in (("weight", w), ("bias", b))},
               tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": l.view(1, -1, 1, 1) for k, l in enumerate(net.lins)}, tmp_path / "lin.pth")
    with pytest.warns(RuntimeWarning, match="UNPINNED"):
        m = lpips.LPIPS(net="vgg", model_path=str(tmp_path / "lin.pth"), vgg_path=str(tmp_path / "vgg16.pth"), verbose=False)
    assert m.to("cuda") is m and m.eval() is m and m.cuda() is m
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(m.convs, net.convs))
    with pytest.raises(NotImplementedError, match="retPerLayer"):
        m(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16), retPerLayer=True)


# ---- checks before any library call ----
def test_arguments_are_checked_before_the_library_is_loaded(monkeypatch):
    from texgs import _lib, lpips as L, metrics
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_bound", {})             # no table counts as applied: entry() would have to load
    net = L.LPIPSVGG.random(2, widths=(16,) * 5)
    ok = torch.zeros(3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(ok, ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.features(ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.lpips(ok, ok, net=net)
    for bad, what in ((torch.zeros(4, 16, 16), "must be"), (torch.zeros(3, 15, 16), "at least 16"), (torch.zeros(16, 16), "must be"),
                      (torch.zeros(3, 16, 16, dtype=torch.float64), "float32"), (torch.zeros(3, 16, 32)[:, :, ::2], "contiguous"),
                      (np.zeros((3, 16, 16), np.float32), "must be")):
        with pytest.raises(ValueError, match=what):
            net(bad, bad)
    with pytest.raises(ValueError, match="one shape"):
        net(ok, torch.zeros(3, 16, 17))
    with pytest.raises(ValueError, match="one shape"):
        net.layers(ok[None], ok)
    with pytest.raises(ValueError, match="one pair"):
        metrics.lpips(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16), net=net)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.conv3x3(torch.zeros(1, 3, 4, 4), torch.zeros(8, dtype=torch.uint8), torch.zeros(16))
    with pytest.raises(ValueError, match="view"):
        L.conv3x3(torch.zeros(1, 3, 4, 8)[:, :, :, ::2], torch.zeros(8, dtype=torch.uint8), torch.zeros(16))      # columns not adjacent
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.conv3x3(torch.zeros(1, 3, 6, 8)[:, :, 1:5, 2:6], torch.zeros(8, dtype=torch.uint8), torch.zeros(16))    # a plane view is a shape it takes
    with pytest.raises(ValueError, match="Cout"):
        L.check_channels(3, 24)
    with pytest.raises(ValueError, match="Cin"):
        L.check_channels(513, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.lpips_head(torch.zeros(2, 16, 3, 3), torch.zeros(16), torch.zeros(1, 8, dtype=torch.float64), 0)
    with pytest.raises(ValueError, match=r"\[2P, C, h, w\]"):
        L.lpips_head(torch.zeros(3, 16, 3, 3), torch.zeros(16), torch.zeros(1, 8, dtype=torch.float64), 0)


def test_metrics_lpips_without_a_net_says_how_to_build_one():
    from texgs import metrics
    metrics.set_lpips(None)
    with pytest.raises(RuntimeError, match=r"LPIPSVGG\(vgg_state, lin_state\)"):
        metrics.lpips(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))
    sentinel = object()
    metrics.set_lpips(sentinel)
    assert metrics._default_lpips is sentinel
    metrics.set_lpips(None)


def test_evaluator_without_a_net_returns_todays_keys():
    from texgs import metrics
    ev = metrics.Evaluator(3)
    assert ev.result() == dict(views=0, l1=None, psnr=None, ssim=None, mae=None)
    assert list(ev.result()) == ["views", "l1", "psnr", "ssim", "mae"] and tuple(ev.rows().shape) == (0, 16)
    with_net = metrics.Evaluator(3, lpips=object())
    assert list(with_net.result()) == ["views", "l1", "psnr", "ssim", "mae", "lpips", "avg_error"]
    assert with_net.result()["lpips"] is None


# ---- the C side without a GPU ----
def test_ctypes_mirrors_match_the_header(tmp_path):
    from texgs import lpips as L
    structs = {"TexGSConv3x3": L.Conv3x3Struct, "TexGSLpipsHead": L.LpipsHeadStruct}
    consts = {"TEXGS_LPIPS_FP32": L.PRECISION["fp32"], "TEXGS_LPIPS_BF16X3": L.PRECISION["bf16x3"], "TEXGS_CONV_TILE_H": L.TILE_H,
              "TEXGS_CONV_TILE_W": L.TILE_W, "TEXGS_CONV_CIN_STEP": L.CIN_STEP, "TEXGS_CONV_K_STEP": L.K_STEP,
              "TEXGS_CONV_COUT_TILE": L.COUT_TILE, "TEXGS_CONV_MAX_CHANNELS": L.MAX_CHANNELS, "TEXGS_CONV_MAX_BATCH": L.MAX_BATCH,
              "TEXGS_LPIPS_ROW": L.ROW, "TEXGS_LPIPS_LAYERS": L.LAYERS, "TEXGS_LPIPS_HEAD_MAX_BLOCKS": L.HEAD_MAX_BLOCKS}
    assert abi_check.layout_mismatches("texgs_lpips.h", structs, consts, tmp_path) == []


def test_every_prototype_has_a_signature_of_the_same_arity(lib_built):
    from texgs import lpips as L
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(L.SIGNATURES) and len(protos) == 5
    assert abi_check.signature_mismatches(HDR, L.SIGNATURES, {"TexGSConv3x3": L.Conv3x3Struct, "TexGSLpipsHead": L.LpipsHeadStruct}) == []
    lib = ctypes.CDLL(lib_built)
    for name in protos:
        assert hasattr(lib, name), name
    from texgs import _lib
    assert _lib.ABI_VERSION == 19 and not set(L.SIGNATURES) & set(_lib.SIGNATURES)


def test_entry_points_refuse_before_any_launch(lib_built):
    """Every refused argument returns an error that names it; nothing is launched (no GPU is needed to see it: a launch here would
    fail with a HIP error that does not name the argument)."""
    import ctypes as C
    from texgs import lpips as L
    lib = L.entry()
    err = lambda: lib.texgs_last_error().decode()
    assert lib.texgs_conv3x3_packed_bytes(3, 64, 0) == 64 * 8 * 9 * 4
    assert lib.texgs_conv3x3_packed_bytes(24, 48, 0) == 64 * 24 * 9 * 4
    assert lib.texgs_conv3x3_packed_bytes(512, 512, 0) == 512 * 512 * 9 * 4
    assert lib.texgs_conv3x3_packed_bytes(64, 24, 0) == 0 and "Cout" in err()
    assert lib.texgs_conv3x3_packed_bytes(513, 64, 0) == 0 and "Cin" in err()
    assert lib.texgs_conv3x3_packed_bytes(0, 64, 0) == 0 and "Cin" in err()
    assert lib.texgs_conv3x3_packed_bytes(64, 528, 0) == 0 and "Cout" in err()
    assert lib.texgs_conv3x3_packed_bytes(64, 64, 1) == 0 and "TEXGS_LPIPS_BF16X3" in err()
    assert lib.texgs_conv3x3_packed_bytes(64, 64, 7) == 0 and "unknown precision 7" in err()
    buf = (C.c_float * 64)()              # stands in for every device pointer: a refused call reads none of them
    b = C.addressof(buf)
    assert lib.texgs_conv3x3_pack(b, 64, 64, 2, b, None) != 0 and "precision" in err()
    assert lib.texgs_conv3x3_pack(None, 64, 64, 0, b, None) != 0 and "NULL" in err()
    assert lib.texgs_conv3x3_pack(b, 64, 64, 0, b + 4, None) != 0 and "16-byte" in err()

    def conv(**kw):
        f = dict(x=b, packed=b, bias=b, in_scale=None, in_shift=None, y=b, B=1, Cin=16, Cout=16, H=4, W=4, relu=1, pool_in=0, precision=0)
        f.update(kw)
        return lib.texgs_conv3x3(C.byref(L.Conv3x3Struct(**f)), None)
    for kw, word in ((dict(Cout=24), "Cout"), (dict(Cin=513), "Cin"), (dict(packed=None), "packed"), (dict(precision=5), "unknown precision"),
                     (dict(precision=1), "BF16X3"), (dict(H=1, pool_in=1), "pool_in"), (dict(W=1, pool_in=1), "pool_in"),
                     (dict(in_scale=b), "in_scale and in_shift"), (dict(in_shift=b), "in_scale and in_shift"), (dict(x=None), "NULL"),
                     (dict(y=None), "NULL"), (dict(bias=None), "NULL"), (dict(B=0), "B must"), (dict(B=65536), "B must"), (dict(H=0), "H and W"),
                     (dict(B=40000, H=256, W=256), "2^31"), (dict(H=1, W=1 << 30), "pixel tiles"), (dict(H=2, W=1 << 29), "pixel tiles"),
                     (dict(x_row=3, x_chan=16, x_img=256), "x_row"), (dict(x_row=4), "x_row"), (dict(x_row=4, x_chan=15, x_img=256), "x_chan"),
                     (dict(x_row=4, x_chan=16, x_img=255), "x_img"), (dict(y_row=4, y_chan=16, y_img=-256), "y_img"),
                     (dict(B=4, y_row=4, y_chan=16, y_img=1 << 61), "y_img"), (dict(y_row=5, y_chan=19, y_img=400), "y_chan"), (dict(relu=2), "relu"), (dict(x=b + 2), "4-byte"), (dict(packed=b + 8), "16-byte")):
        assert lib.texgs_lpips_head_temp_bytes(0, 1, 1) == 0 and "P must" in err()          # another message first
        assert conv(**kw) != 0, kw
        assert word in err(), (kw, err())
    assert lib.texgs_conv3x3(None, None) != 0 and "NULL" in err()

    assert lib.texgs_lpips_head_temp_bytes(3, 37, 41) == 3 * 6 * 8 and lib.texgs_lpips_head_temp_bytes(1, 1, 1) == 8
    assert lib.texgs_lpips_head_temp_bytes(2, 800, 800) == 2 * 1024 * 8
    assert lib.texgs_lpips_head_temp_bytes(1, 0, 4) == 0 and "h and w" in err()
    d64 = (C.c_double * 16)()
    o = C.addressof(d64)

    def head(**kw):
        f = dict(f=b, lin=b, out=o, temp=o, P=1, C=16, h=2, w=2, layer=0)
        f.update(kw)
        return lib.texgs_lpips_head(C.byref(L.LpipsHeadStruct(**f)), None)
    for kw, word in ((dict(P=0), "P must"), (dict(C=0), "C must"), (dict(C=513), "C must"), (dict(layer=5), "layer"), (dict(layer=-1), "layer"),
                     (dict(f=None), "NULL"), (dict(lin=None), "NULL"), (dict(out=None), "NULL"), (dict(temp=None), "NULL"), (dict(h=0), "h and w"),
                     (dict(out=o + 4), "8-byte"), (dict(f=b + 1), "4-byte")):
        assert lib.texgs_conv3x3_packed_bytes(0, 64, 0) == 0 and "Cin" in err()
        assert head(**kw) != 0, kw
        assert word in err(), (kw, err())
