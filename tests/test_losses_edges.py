"""The loss front-end (texgs/losses.py, csrc/loss.hip) at tile edges and degenerate inputs: images smaller than the 11-tap SSIM
window, partial 16x16 tiles combined with the block loop of k_ssim_fwd and the grid-stride loops of k_alpha_l1 / k_geom_sums
(363x367), every term alone with its own gradient, mask=None, the depth-only call, exact ties, near-convergence, constant, dark
and over-range images, fractional masks and a small gamma.

Checker: oracle/losses_torch.py in float64 on the CPU.  tests/golden/loss_edges.npz pins that restatement to the reference's own
functions (float32, with autograd) at the shapes below the window size and at the tie / near-convergence values.

How a gradient (or a normal map) is judged: per pixel against float64, reported for the border ring and the interior separately
(`loss_edges/...` lines of helpers.report), relative to scale = max(max|g64|, 1/(C*H*W)); the second term keeps the check
meaningful where the true gradient is ~0.  The bar of a case is max(16 x the error of the float32 CPU restatement against float64,
1e-5 x scale), never looser than 1e-3 x scale: the restatement's own rounding, not the code under test, sets it; the factor 16
allows for the kernels' reordering of the same fp32 arithmetic (separable 11 + 11 taps instead of 121, a reciprocal, __expf)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import losses_torch as LO

E = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_edges.npz")
RGB_GOLDEN = ["1x1", "1x9", "9x1", "5x7", "17x31"]
GEOM_GOLDEN = ["1x1", "1x9", "9x1", "2x2", "17x15"]
LAMS = {"l0": 0.0, "l1": 1.0, "l02": 0.2}
GAMMAS = {"g01": 0.1, "g001": 0.01}
LA = 0.1
BIG = "363x367"      # 23 x 23 x 3 = 1587 tile jobs > 1024 blocks, every last row / column a partial tile; P = 133221 > 512 * 256, P % 256 = 101


def _hw(shp):
    return tuple(int(v) for v in shp.split("x"))


@functools.lru_cache(maxsize=None)
def _fixture():
    d = np.load(E)
    return {k: d[k] for k in d.files}


def _scale(g64):
    return max(float(g64.abs().max()), 1.0 / g64.numel())


def _ring(H, W, r):
    ring = torch.ones(H, W, dtype=torch.bool)
    if H > 2 * r and W > 2 * r:
        ring[r:H - r, r:W - r] = False
    return ring


def _bar(g64, g32):
    """max(16 x the float32 restatement's own error, 1e-5 x scale), capped at the suite's 1e-3 x scale."""
    scale = _scale(g64)
    base = float((g32.double() - g64).abs().max())
    return min(max(16.0 * base, 1e-5 * scale), 1e-3 * scale), base, scale


def _compare(label, got, g64, g32, r):
    """Per-pixel comparison of a [C,H,W] map with float64: border ring of width r and interior apart; reported, then asserted."""
    import helpers as Hh
    _, H, W = g64.shape
    bar, base, scale = _bar(g64, g32)
    err = (got.detach().cpu().double() - g64).abs().amax(dim=0)
    ring = _ring(H, W, r)
    eb = float(err[ring].max())
    ei = float(err[~ring].max()) if bool((~ring).any()) else 0.0
    Hh.report(f"loss_edges/{label}", border_abs=eb, border_rel=eb / scale, interior_abs=ei, interior_rel=ei / scale,
              bar_rel=bar / scale, fp32_restatement_rel=base / scale, scale=scale)
    assert max(eb, ei) <= bar, (label, eb, ei, bar)


def _report_value(label, loss, l64, bar):
    import helpers as Hh
    Hh.report(f"loss_edges/{label}/loss", loss_abs=abs(loss - l64), bar_abs=bar, loss=l64)


# ------------------------------------------------------------------------------------------------------------ inputs, references
def _ties_block(t, gt):
    _, H, W = t.shape
    if H * W > 1:
        t[:, :(H + 1) // 2, :(W + 1) // 2] = gt[:, :(H + 1) // 2, :(W + 1) // 2]
    return t


@functools.lru_cache(maxsize=None)
def _rgb_inputs(case):
    """-> img, gt, alpha, gta (float32, CPU).  `case` is a shape (the fixture's inputs where it holds that shape) or a value regime
    at 37x45.  Alpha equals gt_alpha on a block in every case: a saturated alpha map."""
    if case in RGB_GOLDEN:
        d = _fixture()
        return tuple(torch.tensor(d[f"rgb{case}_{k}"]) for k in ("img", "gt", "alpha", "gta"))
    H, W = _hw(case) if "x" in case else (37, 45)
    g = torch.Generator().manual_seed(1000 * H + W + sum(map(ord, case)))
    gt = torch.rand(3, H, W, generator=g)
    img = torch.rand(3, H, W, generator=g)
    if case == "equal":
        img = gt.clone()
    elif case == "equal_left":
        img[:, :, :W // 2] = gt[:, :, :W // 2]
    elif case == "near":
        img = gt + 1e-3 * torch.randn(3, H, W, generator=g)
    elif case == "smooth":
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        gt = torch.stack([0.5 + 0.4 * torch.sin(3 * xx + c) * torch.cos(2 * yy - c) for c in range(3)])
        img = gt + 1e-2 * torch.randn(3, H, W, generator=g)
    elif case == "const1":
        img, gt = torch.ones(3, H, W), torch.ones(3, H, W)
    elif case == "const05_noise":
        img = torch.full((3, H, W), 0.5)
    elif case == "zeros_noise":
        img = torch.zeros(3, H, W)
    elif case == "dark":
        img, gt = img * 0.02, gt * 0.02
    elif case == "bright":
        img, gt = img * 4.0, gt * 4.0
    elif case == "overrange":
        img, gt = img * 1.5 - 0.2, gt * 1.5 - 0.2
    gta = (torch.rand(1, H, W, generator=g) > 0.4).float()
    alpha = _ties_block(torch.rand(1, H, W, generator=g), gta)
    return img, gt, alpha, gta


def _grad(fn, dtype, *leaves):
    ls = [t.detach().to(dtype).clone().requires_grad_(True) for t in leaves]        # never the shared input itself
    loss = fn(*ls)
    loss.backward()
    return (float(loss.detach()),) + tuple(t.grad for t in ls)


@functools.lru_cache(maxsize=None)
def _rgb_ref(case, lam, la):
    """float64 and float32 restatement: loss64, dimg64, dimg32, dalpha64, dalpha32."""
    img, gt, alpha, gta = _rgb_inputs(case)
    res = []
    for dt in (torch.float64, torch.float32):
        if la:
            res.append(_grad(lambda i, a: LO.rgb_alpha_loss(i, gt.to(dt), a, gta.to(dt), lam, la), dt, img, alpha))
        else:
            res.append(_grad(lambda i: LO.rgb_alpha_loss(i, gt.to(dt), None, None, lam, 0.0), dt, img) + (None,))
    (l64, gi64, ga64), (_, gi32, ga32) = res
    return l64, gi64, gi32, ga64, ga32


def _piecewise_normals(H, W, g):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    n = (torch.randn(3, H // 3 + 1, W // 3 + 1, generator=g) * 0.5).repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W]
    return n * ((xx + yy) < 2 * (H + W) // 3).float()


@functools.lru_cache(maxsize=None)
def _geom_inputs(shp, gti_kind="blocks"):
    """-> norm, gtn, gti, fractional mask, depth, gtd.  Piecewise-constant normals with a zero region (ties in the smoothness term,
    as a render has on the background), depth equal to gt_depth on a block."""
    if shp in GEOM_GOLDEN and gti_kind == "blocks":
        d = _fixture()
        return tuple(torch.tensor(d[f"geo{shp}_{k}"]) for k in ("norm", "gtn", "gti", "mask", "depth", "gtd"))
    H, W = _hw(shp)
    g = torch.Generator().manual_seed(7000 * H + W + len(gti_kind))
    norm = _piecewise_normals(H, W, g)
    gtn = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    if gti_kind == "blocks":
        gti = (torch.rand(3, H // 6 + 1, W // 6 + 1, generator=g).repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :H, :W]
               + 0.05 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
    elif gti_kind == "smooth":            # neighbours differ by ~1e-2: weights near 1 at gamma 0.1
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        gti = torch.stack([0.5 + 0.4 * torch.sin(3 * xx + c) * torch.cos(2 * yy - c) for c in range(3)])
    else:                                 # "noisy": neighbours differ by ~1: weights near 0 at gamma 0.01
        gti = torch.rand(3, H, W, generator=g)
    mask = torch.rand(1, H, W, generator=g) * (torch.rand(1, H, W, generator=g) > 0.25).float()
    gtd = 3.0 + torch.rand(1, H, W, generator=g)
    depth = _ties_block(3.0 + torch.rand(1, H, W, generator=g), gtd)
    return norm, gtn, gti, mask, depth, gtd


def _mask_of(kind, mask):
    return {"fractional": mask, "binary": (mask > 0.3).float(), "none": None}[kind]


def _geom_ref(shp, gti_kind, mask_kind, ln, ls, ld, gamma):
    """float64 and float32 restatement: loss64, dnorm64, dnorm32, ddepth64, ddepth32.  mask=None: norm_loss(mask=None) and the
    smoothness term with a mask of ones (the reference's smooth_loss cannot take None)."""
    norm, gtn, gti, mask, depth, gtd = _geom_inputs(shp, gti_kind)
    m = _mask_of(mask_kind, mask)
    res = []
    for dt in (torch.float64, torch.float32):
        mm = None if m is None else m.to(dt)
        ones = torch.ones(1, *norm.shape[1:], dtype=dt) if m is None else mm

        def fn(n, z):
            loss = ld * (z - gtd.to(dt)).abs().mean()
            if ln:
                loss = loss + ln * LO.norm_loss(n, gtn.to(dt), mm)
            if ls:
                loss = loss + ls * LO.smooth_loss(gti.to(dt), n, ones, gamma)
            return loss + 0.0 * n.sum()
        res.append(_grad(fn, dt, norm, depth))
    (l64, gn64, gd64), (_, gn32, gd32) = res
    return l64, gn64, gn32, gd64, gd32


# ---------------------------------------------------------------------------------- CPU: the restatement against the reference
@pytest.mark.parametrize("shp", RGB_GOLDEN)
def test_restatement_matches_reference_loss_edges(shp):
    """Same tolerances as test_restatement_matches_reference_losses, with an absolute floor of 1e-5 x scale on the gradients
    (tie regions, where the true gradient is ~0 and rtol says nothing)."""
    d = _fixture()
    img, gt, alpha, gta = _rgb_inputs(shp)
    assert abs(float(LO.ssim(img.double(), gt.double())) - float(d[f"rgb{shp}_ssim"])) < 2e-6
    assert abs(float((img.double() - gt.double()).abs().mean()) - float(d[f"rgb{shp}_Ll1"])) < 2e-6
    for name, lam in LAMS.items():
        l64, gi64, _, ga64, _ = _rgb_ref(shp, lam, LA)
        ref = (1.0 - lam) * float(d[f"rgb{shp}_Ll1"]) + lam * (1.0 - float(d[f"rgb{shp}_ssim"])) + LA * float(d[f"rgb{shp}_Lalpha"])
        assert abs(l64 - ref) < 2e-6
        assert np.allclose(gi64.numpy(), d[f"rgb{shp}_dimg_{name}"], atol=max(2e-8, 1e-5 * _scale(gi64)), rtol=1e-4), name
        assert np.allclose(ga64.numpy(), LA * d[f"rgb{shp}_dalpha"], atol=1e-9)
    if shp == "5x7":        # the fixture does hold the tie regimes
        assert bool((img[:, :, :3] == gt[:, :, :3]).all()) and bool((alpha[:, :3, :4] == gta[:, :3, :4]).all())
        assert float(np.abs(d["rgb5x7_dimg_l0"][:, :, :3]).max()) == 0.0 and float(np.abs(d["rgb5x7_dalpha"][:, :3, :4]).max()) == 0.0


@pytest.mark.parametrize("shp", GEOM_GOLDEN)
def test_geom_restatement_matches_reference_loss_edges(shp):
    """Same tolerances as test_geom_restatement_matches_reference_losses, each term alone, with the 1e-5 x scale floor."""
    d = _fixture()
    t = f"geo{shp}"
    l64, gn64, _, _, _ = _geom_ref(shp, "blocks", "fractional", 1.0, 0.0, 0.0, 0.1)
    assert abs(l64 - float(d[f"{t}_Lnorm"])) < 2e-6
    assert np.allclose(gn64.numpy(), d[f"{t}_dnorm_n"], atol=max(1e-8, 1e-5 * _scale(gn64)), rtol=2e-4)
    for name, gamma in GAMMAS.items():
        l64, gn64, _, _, _ = _geom_ref(shp, "blocks", "fractional", 0.0, 1.0, 0.0, gamma)
        assert abs(l64 - float(d[f"{t}_Lnsm_{name}"])) < 2e-6
        assert np.allclose(gn64.numpy(), d[f"{t}_dnorm_s_{name}"], atol=max(1e-8, 1e-5 * _scale(gn64)), rtol=2e-4), name
    l64, _, _, gd64, _ = _geom_ref(shp, "blocks", "fractional", 0.0, 0.0, 1.0, 0.1)
    assert abs(l64 - float(d[f"{t}_Ld"])) < 2e-6
    assert np.allclose(gd64.numpy(), d[f"{t}_ddepth"], atol=1e-9)
    if shp == "17x15":      # ties: zero region and constant blocks in the normals, depth == gt_depth on a block
        norm, _, _, _, depth, gtd = _geom_inputs(shp)
        assert float(norm[:, 12:, 12:].abs().max()) == 0.0 and bool((norm[:, 0, 0] == norm[:, 2, 2]).all())
        assert bool((depth[:, :9, :8] == gtd[:, :9, :8]).all()) and float(np.abs(d[f"{t}_ddepth"][:, :9, :8]).max()) == 0.0


# ------------------------------------------------------------------------------ CPU: shapes are validated before anything is launched
def _cpu_maps(H=6, W=7):
    g = torch.Generator().manual_seed(1)
    r = lambda c, h=H, w=W: torch.rand(c, h, w, generator=g)
    return r


def test_rgb_alpha_loss_rejects_mis_sized_maps_without_a_gpu():
    """A map of another resolution would be read out of bounds by the kernels: it must raise before the library is even loaded
    (CPU tensors here, so nothing can reach a kernel); a well-shaped call goes on to the missing-CPU-fallback error."""
    from texgs.losses import rgb_alpha_loss
    r = _cpu_maps()
    img, gt, a, ga = r(3), r(3), r(1), r(1)
    with pytest.raises(ValueError, match="gt_image"):
        rgb_alpha_loss(img, r(3, 6, 8))
    with pytest.raises(ValueError, match="image"):
        rgb_alpha_loss(r(1), r(1))
    with pytest.raises(ValueError, match=r"alpha.*\(1, 3, 7\)"):
        rgb_alpha_loss(img, gt, r(1, 3, 7), ga, lambda_alpha=0.1)
    with pytest.raises(ValueError, match=r"gt_alpha.*\(1, 12, 14\)"):
        rgb_alpha_loss(img, gt, a, r(1, 12, 14), lambda_alpha=0.1)
    with pytest.raises(ValueError, match="gt_alpha is None"):          # a non-zero lambda needs both maps of its term
        rgb_alpha_loss(img, gt, a, None, lambda_alpha=0.1)
    with pytest.raises(ValueError, match="alpha is None"):
        rgb_alpha_loss(img, gt, lambda_alpha=0.1)
    for ok in (dict(), dict(alpha=a, gt_alpha=ga, lambda_alpha=0.1), dict(alpha=a[0], gt_alpha=ga[0], lambda_alpha=0.1),
               dict(alpha=r(1, 3, 7), gt_alpha=ga, lambda_alpha=0.0)):           # [H,W] for [1,H,W]; a zero lambda reads nothing
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rgb_alpha_loss(img, gt, **ok)


def test_geom_losses_rejects_mis_sized_maps_without_a_gpu():
    from texgs.losses import geom_losses
    r = _cpu_maps()
    n, gn, gi, m, z, gz = r(3), r(3), r(3), r(1), r(1), r(1)
    bad = [("mask", dict(norm=n, gt_norm=gn, mask=r(1, 3, 7), lambda_norm=1.0)),
           ("mask", dict(norm=n, gt_image=gi, mask=r(1, 12, 14), lambda_smooth=1.0)),
           ("gt_norm", dict(norm=n, gt_norm=r(3, 6, 6), lambda_norm=1.0)),
           ("gt_norm", dict(norm=n, lambda_norm=1.0)),
           ("gt_image", dict(norm=n, gt_image=r(1), lambda_smooth=1.0)),
           ("norm", dict(norm=r(2), gt_norm=gn, lambda_norm=1.0)),
           ("norm", dict(gt_norm=gn, lambda_norm=1.0)),
           ("gt_depth", dict(depth=z, gt_depth=r(1, 6, 8), lambda_depth=1.0)),
           ("gt_depth is None", dict(depth=z, lambda_depth=1.0)),
           ("depth is None", dict(norm=n, gt_norm=gn, gt_depth=gz, lambda_norm=1.0, lambda_depth=1.0)),
           ("depth", dict(norm=n, gt_norm=gn, depth=r(1, 7, 6), gt_depth=r(1, 7, 6), lambda_norm=1.0, lambda_depth=1.0)),
           ("depth", dict(norm=n, gt_norm=gn, depth=r(1, 3, 7), gt_depth=gz, lambda_norm=1.0, lambda_depth=1.0))]
    for name, kw in bad:
        with pytest.raises(ValueError, match=name):
            geom_losses(**kw)
    good = [dict(norm=n, gt_norm=gn, mask=m, lambda_norm=1.0), dict(norm=n, gt_norm=gn, mask=m[0], lambda_norm=1.0),
            dict(norm=n, gt_image=gi, lambda_smooth=1.0), dict(depth=z, gt_depth=gz[0], lambda_depth=1.0),
            dict(norm=n, gt_norm=gn, gt_image=gi, mask=m, depth=z, gt_depth=gz, lambda_norm=0.1, lambda_smooth=0.5, lambda_depth=0.3),
            # tensors of a term whose lambda is 0 are not read, hence not checked
            dict(norm=n, gt_norm=gn, gt_image=r(3, 2, 2), depth=r(1, 9, 9), gt_depth=gz, lambda_norm=1.0),
            dict(norm=r(3, 2, 2), gt_norm=gn, mask=r(1, 2, 2), depth=z, gt_depth=gz, lambda_depth=1.0)]
    for kw in good:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            geom_losses(**kw)
    # a map left on another device than the one the kernels run on is a host pointer in a kernel: refused by name as well
    from texgs.losses import _check_device
    with pytest.raises(ValueError, match="mask is on cpu"):
        _check_device(torch.device("cuda:0"), gt_norm=None, mask=m)


# ------------------------------------------------------------------------------------------------------------- GPU: rgb_alpha_loss
def _hip_rgb(case, lam, la):
    from texgs.losses import rgb_alpha_loss
    img, gt, alpha, gta = _rgb_inputs(case)
    dev = torch.device("cuda:0")
    i = img.to(dev).requires_grad_(True)
    a = alpha.to(dev).requires_grad_(True) if la else None
    loss = rgb_alpha_loss(i, gt.to(dev), a, gta.to(dev) if la else None, lam, la)
    loss.backward()
    return float(loss.detach()), i.grad, (a.grad if la else None)


def _check_rgb(case, name, lam, la, value_bar=3e-6):
    l64, gi64, gi32, ga64, ga32 = _rgb_ref(case, lam, la)
    loss, gi, ga = _hip_rgb(case, lam, la)
    label = f"rgb/{case}/{name}" + ("_alpha" if la else "")
    _report_value(label, loss, l64, value_bar)
    _compare(label + "/dimg", gi, gi64, gi32, 5)
    if la:
        _compare(label + "/dalpha", ga, ga64, ga32, 5)
    assert abs(loss - l64) < value_bar, (case, name, loss, l64)
    return loss


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAMS))
@pytest.mark.parametrize("shp", ["1x1", "1x9", "9x1", "5x7", "11x11", "15x17", "16x16", "17x31", "33x16", BIG])
def test_hip_rgb_alpha_loss_shapes(lib_built, shp, name):
    """lambda_dssim 0 (L1 alone), 1 (SSIM alone) and 0.2 at every shape; with the alpha term at 5x7, 17x31 and 363x367."""
    lam = LAMS[name]
    d = _fixture()
    bar = 5e-6 if shp == BIG else 3e-6
    la = LA if shp in ("5x7", "17x31", BIG) else 0.0
    loss = _check_rgb(shp, name, lam, la, bar)
    t = f"rgb{shp}"
    if shp in RGB_GOLDEN:
        ref = (1.0 - lam) * float(d[f"{t}_Ll1"]) + lam * (1.0 - float(d[f"{t}_ssim"])) + la * float(d[f"{t}_Lalpha"])
        assert abs(loss - ref) < 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["equal", "equal_left", "near", "smooth", "const1", "const05_noise", "zeros_noise", "dark", "bright",
                                    "overrange"])
def test_hip_rgb_alpha_loss_value_regimes(lib_built, regime):
    """37x45 (partial tiles on both axes).  All three lambdas; the alpha term (exact ties on a block) rides along at 0.2."""
    for name, lam in LAMS.items():
        _check_rgb(regime, name, lam, LA if name == "l02" else 0.0)


@pytest.mark.gpu
def test_hip_rgb_alpha_loss_upstream_gradient_and_second_backward(lib_built):
    """backward of 3.5 * loss, twice over the same graph: the stored gradient is scaled out of place."""
    from texgs.losses import rgb_alpha_loss
    case = "equal_left"
    img, gt, alpha, gta = _rgb_inputs(case)
    _, gi64, gi32, ga64, ga32 = _rgb_ref(case, 0.2, LA)
    dev = torch.device("cuda:0")
    i, a = img.to(dev).requires_grad_(True), alpha.to(dev).requires_grad_(True)
    loss = 3.5 * rgb_alpha_loss(i, gt.to(dev), a, gta.to(dev), 0.2, LA)
    loss.backward(retain_graph=True)
    g1, a1 = i.grad.clone(), a.grad.clone()
    _compare("rgb/upstream3.5/dimg", g1 / 3.5, gi64, gi32, 5)
    _compare("rgb/upstream3.5/dalpha", a1 / 3.5, ga64, ga32, 5)
    loss.backward()
    assert torch.equal(i.grad, 2.0 * g1) and torch.equal(a.grad, 2.0 * a1)


@pytest.mark.gpu
def test_hip_rgb_alpha_loss_non_contiguous_image(lib_built):
    """A CHW view of an HWC tensor against its contiguous copy: bit-identical gradient; bit-identical loss where that is a defined
    property.  The loss is the sum of per-block partial sums added with float atomics in no fixed order (k_ssim_fwd's last line),
    so two runs of the SAME input may differ in the last bit once three different partial sums meet; d_img does not depend on
    those sums.  With equal channels (one 13x15 tile per channel, three equal partial sums) every order gives the same bits.  The
    colour 37x45 case is held to the gradient and the value bar.  Measured on an MI355X, not only read from the code: 2000 calls on
    ONE colour 37x45 input gave 4 distinct float32 loss values (3 ulp apart at most), 500 calls at 363x367 gave 7."""
    from texgs.losses import rgb_alpha_loss
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(77)
    grey = torch.rand(13, 15, 1, generator=g).expand(13, 15, 3).contiguous(), torch.rand(1, 13, 15, generator=g).expand(3, 13, 15)
    img, gt, _, _ = _rgb_inputs("equal_left")
    colour = img.permute(1, 2, 0).contiguous(), gt
    for tag, (hwc, gt) in (("grey", grey), ("colour", colour)):
        res = []
        for view in (True, False):
            i = hwc.to(dev).permute(2, 0, 1)
            assert not i.is_contiguous()
            i = (i if view else i.contiguous()).requires_grad_(True)
            loss = rgb_alpha_loss(i, gt.to(dev), None, None, 0.2, 0.0)
            loss.backward()
            res.append((loss.detach(), i.grad))
        assert torch.equal(res[0][1], res[1][1]), tag
        if tag == "grey":
            assert torch.equal(res[0][0], res[1][0])
        else:
            assert abs(float(res[0][0]) - float(res[1][0])) < 3e-6


@pytest.mark.gpu
def test_hip_rgb_alpha_loss_on_two_streams(lib_built):
    from texgs.losses import rgb_alpha_loss
    case = "smooth"
    dev = torch.device("cuda:0")
    img, gt, alpha, gta = (t.to(dev) for t in _rgb_inputs(case))
    l64 = _rgb_ref(case, 0.2, LA)[0]

    def run():
        i, a = img.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
        loss = rgb_alpha_loss(i, gt, a, gta, 0.2, LA)
        loss.backward()                                   # upstream gradient 1: i.grad IS d_img, a.grad IS d_a
        return loss.detach(), i.grad, a.grad
    base = run()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    res = []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            res.append(run())
    torch.cuda.synchronize()
    assert abs(float(base[0]) - l64) < 3e-6
    for loss, gi, ga in res:
        assert torch.equal(gi, base[1]) and torch.equal(ga, base[2])
        assert abs(float(loss) - l64) < 3e-6


# --------------------------------------------------------------------------------------------------------------- GPU: geom_losses
def _hip_geom(shp, gti_kind, mask_kind, ln, ls, ld, gamma, with_norm=True):
    from texgs.losses import geom_losses
    norm, gtn, gti, mask, depth, gtd = _geom_inputs(shp, gti_kind)
    dev = torch.device("cuda:0")
    m = _mask_of(mask_kind, mask)
    n = norm.to(dev).requires_grad_(True) if with_norm else None
    z = depth.to(dev).requires_grad_(True) if ld else None
    loss = geom_losses(norm=n, gt_norm=gtn.to(dev) if ln else None, gt_image=gti.to(dev) if ls else None,
                       mask=None if m is None or not with_norm else m.to(dev), depth=z, gt_depth=gtd.to(dev) if ld else None,
                       lambda_norm=ln, lambda_smooth=ls, gamma=gamma, lambda_depth=ld)
    loss.backward()
    return float(loss.detach()), (n.grad if with_norm and (ln or ls) else None), (z.grad if ld else None)


def _check_geom(label, shp, gti_kind, mask_kind, ln, ls, ld, gamma, value_bar, golden=None, with_norm=True):
    l64, gn64, gn32, gd64, gd32 = _geom_ref(shp, gti_kind, mask_kind, ln, ls, ld, gamma)
    loss, gn, gd = _hip_geom(shp, gti_kind, mask_kind, ln, ls, ld, gamma, with_norm)
    _report_value(f"geom/{label}", loss, l64, value_bar)
    if ln or ls:
        _compare(f"geom/{label}/dnorm", gn, gn64, gn32, 1)
    if ld:
        _compare(f"geom/{label}/ddepth", gd, gd64, gd32, 1)
    assert abs(loss - l64) < value_bar, (label, loss, l64)
    if golden is not None:
        assert abs(loss - golden) < 3e-6, (label, loss, golden)


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["binary", "fractional", "none"])
@pytest.mark.parametrize("shp", ["1x1", "1x9", "9x1", "2x2", "17x15", "21x27", BIG])
def test_hip_geom_losses_shapes_masks_terms(lib_built, shp, mask_kind):
    """Each term alone (value and gradient), all three together and the depth-only call without `norm`, at gamma 0.1 and 0.01.
    W = 1 or H = 1 leaves at most one pair direction inside the image: sum w = 0 and the 1e-6 alone is the denominator."""
    d = _fixture()
    bar = 5e-6 if shp == BIG else 3e-6
    gold = (lambda k: float(d[f"geo{shp}_{k}"])) if shp in GEOM_GOLDEN and mask_kind == "fractional" else (lambda k: None)
    lab = f"{shp}/{mask_kind}"
    _check_geom(f"{lab}/norm_only", shp, "blocks", mask_kind, 1.0, 0.0, 0.0, 0.1, bar, gold("Lnorm"))
    _check_geom(f"{lab}/depth_only_no_norm", shp, "blocks", mask_kind, 0.0, 0.0, 1.0, 0.1, bar, gold("Ld"), with_norm=False)
    for name, gamma in GAMMAS.items():
        _check_geom(f"{lab}/smooth_only_{name}", shp, "blocks", mask_kind, 0.0, 1.0, 0.0, gamma, bar, gold(f"Lnsm_{name}"))
        _check_geom(f"{lab}/all_{name}", shp, "blocks", mask_kind, 0.1, 0.5, 0.3, gamma, bar)


@pytest.mark.gpu
@pytest.mark.parametrize("gti_kind", ["smooth", "noisy"])
@pytest.mark.parametrize("shp", ["21x27", BIG])
def test_hip_geom_losses_gt_image_regimes(lib_built, shp, gti_kind):
    """A smooth gt image (bilateral weights near 1) and a noisy one (weights near 0 at gamma 0.01: sum w is comparable to, or far
    below, the 1e-6 of the denominator), fractional mask."""
    for name, gamma in GAMMAS.items():
        _check_geom(f"{shp}/{gti_kind}/smooth_only_{name}", shp, gti_kind, "fractional", 0.0, 1.0, 0.0, gamma, 5e-6 if shp == BIG else 3e-6)


# ------------------------------------------------------------------------------------------- GPU: norm_from_depth / norm_reg_loss
TANX, TANY = math.tan(0.35), math.tan(0.30)


@functools.lru_cache(maxsize=None)
def _depth_scene(shp):
    """A tilted, gently bumpy surface with two depth steps, built so that every mask decision sits away from the threshold: depth
    (float32), view matrix (transposed, as the reference stores it), threshold, float64 normals and mask."""
    H, W = _hw(shp)
    y, x = torch.meshgrid(torch.linspace(-1, 1, H, dtype=torch.float64) if H > 1 else torch.zeros(1, dtype=torch.float64),
                          torch.linspace(-1, 1, W, dtype=torch.float64) if W > 1 else torch.zeros(1, dtype=torch.float64), indexing="ij")
    depth = 2.0 + 0.25 * x - 0.15 * y + 0.05 * torch.sin(3 * x + 1) * torch.cos(2 * y)
    if H > 4 and W > 4:
        depth[:, W // 2:] += 0.4
        depth[H // 3:, :] += 0.3
    depth = depth.float().reshape(1, H, W)
    def rot(i, j, a):                   # rotation by a in the (i, j) plane: [i,i] = [j,j] = cos, [i,j] = -sin, [j,i] = sin
        m = torch.eye(3, dtype=torch.float64)
        m[i, i] = m[j, j] = math.cos(a)
        m[i, j], m[j, i] = -math.sin(a), math.sin(a)
        return m
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = rot(0, 1, 1.1) @ rot(2, 0, -0.7) @ rot(1, 2, 0.4)          # Rz(1.1) Ry(-0.7) Rx(0.4)
    view[:3, 3] = torch.tensor([0.3, -0.2, 1.5], dtype=torch.float64)
    wvt = view.t().contiguous()
    lens = _side_lengths(depth.double(), wvt)
    nz = lens[lens > 0]
    thr = 3.0 * float(nz.median()) if nz.numel() else 1e-2
    n64, m64 = LO.norm_from_depth(depth.double(), wvt, TANX, TANY, thr)
    return depth, wvt.float(), thr, n64, m64, lens


def _side_lengths(depth64, wvt64):
    """The four one-sided difference lengths the restatement's mask compares with the threshold, float64: [4,H,W]."""
    return torch.stack([g.norm(dim=0) for g in LO.one_sided_differences(depth64, wvt64, TANX, TANY)])


NFD_SHAPES = ["1x1", "1x9", "9x1", "2x2", "17x15", "33x24", "61x67"]


@pytest.mark.parametrize("shp", NFD_SHAPES)
def test_depth_scene_keeps_mask_decisions_off_the_threshold(shp):
    """Preconditions of the exact-mask GPU test, on the float64 restatement alone (and the float32 restatement agrees)."""
    depth, wvt, thr, n64, m64, lens = _depth_scene(shp)
    H, W = _hw(shp)
    assert float(((lens - thr).abs() < 0.02 * thr).double().mean()) == 0.0
    if H > 4 and W > 4:
        assert 0.5 < float(m64.mean()) < 1.0
    assert bool((m64 == (lens < thr).all(dim=0, keepdim=True).double()).all())
    n32, m32 = LO.norm_from_depth(depth, wvt, TANX, TANY, thr)
    assert bool((m32.double() == m64).all())
    if W == 1 or H == 1:        # one of the two central differences is zero: zero cross product, the 1e-6 clamp gives normal 0
        assert float(n64.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shp", NFD_SHAPES)
def test_hip_norm_from_depth_exact_mask_and_normals(lib_built, shp):
    """No mask decision is within 2 % of the threshold (test above), so the HIP mask equals the float64 mask at EVERY pixel and the
    normals are compared at every pixel; then norm_reg_loss end to end with a fractional gt_alpha, its value held to 3e-6."""
    from texgs.losses import norm_from_depth, norm_reg_loss
    depth, wvt, thr, n64, m64, _ = _depth_scene(shp)
    H, W = _hw(shp)
    dev = torch.device("cuda:0")
    n32, _ = LO.norm_from_depth(depth, wvt, TANX, TANY, thr)
    norm2, mask = norm_from_depth(depth.to(dev), wvt, TANX, TANY, thr)
    assert norm2.shape == (3, H, W) and mask.shape == (1, H, W)
    assert bool((mask.cpu().double() == m64).all()), float((mask.cpu().double() != m64).double().mean())
    _compare(f"norm_from_depth/{shp}/normal", norm2, n64, n32, 1)
    g = torch.Generator().manual_seed(H * 100 + W)
    pred = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    gta = torch.rand(1, H, W, generator=g)
    ref = []
    for dt in (torch.float64, torch.float32):
        ref.append(_grad(lambda p: LO.norm_reg_loss(p, depth.to(dt), wvt.to(dt), TANX, TANY, gta.to(dt), thr), dt, pred))
    (l64, g64), (_, g32) = ref
    p = pred.to(dev).requires_grad_(True)
    loss = norm_reg_loss(p, depth.to(dev), wvt.to(dev), TANX, TANY, gta.to(dev), thr)
    loss.backward()
    loss = float(loss.detach())
    _report_value(f"norm_reg_loss/{shp}", loss, l64, 3e-6)
    _compare(f"norm_reg_loss/{shp}/dnorm", p.grad, g64, g32, 1)
    assert abs(loss - l64) < 3e-6
