"""Fused loss front-end.  PINNED parity: tests/golden/loss_frontend.npz was produced by the reference's
own losses/ functions and their autograd.  CPU: the torch restatement vs the golden.  GPU: the HIP kernels vs the golden
(values within 2e-6, gradients within 1e-7 absolute ~ 1e-3 of their scale) and vs the restatement at 800x800."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import losses_torch as LO

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_frontend.npz")


def _load(tag):
    d = np.load(G)
    t = lambda k: torch.tensor(d[f"{tag}_{k}"])
    return d, t("img"), t("gt"), t("alpha"), t("gta")


@pytest.mark.parametrize("tag", ["s", "m"])
def test_restatement_matches_reference_losses(tag):
    d, img, gt, alpha, gta = _load(tag)
    i64 = img.double().requires_grad_(True)
    a64 = alpha.double().requires_grad_(True)
    loss = LO.rgb_alpha_loss(i64, gt.double(), a64, gta.double(), float(d["lam"]), float(d["la"]))
    loss.backward()
    assert abs(float(loss) - float(d[f"{tag}_loss"])) < 2e-6
    assert abs(float(LO.ssim(img.double(), gt.double())) - float(d[f"{tag}_ssim"])) < 2e-6
    assert np.allclose(i64.grad.numpy(), d[f"{tag}_dimg"], atol=2e-8, rtol=1e-4)
    assert np.allclose(a64.grad.numpy(), d[f"{tag}_dalpha"], atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["s", "m"])
def test_hip_loss_matches_reference_golden(lib_built, tag):
    from texgs.losses import rgb_alpha_loss
    d, img, gt, alpha, gta = _load(tag)
    dev = torch.device("cuda:0")
    i = img.to(dev).requires_grad_(True)
    a = alpha.to(dev).requires_grad_(True)
    loss = rgb_alpha_loss(i, gt.to(dev), a, gta.to(dev), float(d["lam"]), float(d["la"]))
    loss.backward()
    assert abs(float(loss) - float(d[f"{tag}_loss"])) < 3e-6
    gi = d[f"{tag}_dimg"]
    assert float(np.abs(i.grad.cpu().numpy() - gi).max()) < 1e-3 * float(np.abs(gi).max())
    assert np.allclose(a.grad.cpu().numpy(), d[f"{tag}_dalpha"], atol=1e-9)


@pytest.mark.gpu
def test_hip_loss_full_size_vs_restatement(lib_built):
    from texgs.losses import rgb_alpha_loss
    g = torch.Generator().manual_seed(5)
    H = W = 800
    img = torch.rand(3, H, W, generator=g)
    gt = torch.rand(3, H, W, generator=g)
    dev = torch.device("cuda:0")
    i = img.to(dev).requires_grad_(True)
    loss = rgb_alpha_loss(i, gt.to(dev), None, None, 0.2, 0.0)
    (2.0 * loss).backward()
    i64 = img.double().requires_grad_(True)
    ref = LO.rgb_alpha_loss(i64, gt.double(), None, None, 0.2, 0.0)
    (2.0 * ref).backward()
    assert abs(float(loss) - float(ref)) < 5e-6
    assert float((i.grad.cpu().double() - i64.grad).abs().max()) < 1e-3 * float(i64.grad.abs().max())


# ---- geometric regularisers (normal loss, bilateral normal smoothness, depth L1): models/texture_gaussian3d.py:347-368
GG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geom_losses.npz")


def _gload(tag):
    d = np.load(GG)
    t = lambda k: torch.tensor(d[f"{tag}_{k}"])
    return d, t("norm"), t("gtn"), t("gti"), t("mask"), t("depth"), t("gtd")


@pytest.mark.parametrize("tag", ["s", "m"])
def test_geom_restatement_matches_reference_losses(tag):
    d, norm, gtn, gti, mask, depth, gtd = _gload(tag)
    n64 = norm.double().requires_grad_(True)
    d64 = depth.double().requires_grad_(True)
    loss = LO.geom_losses(n64, gtn.double(), gti.double(), mask.double(), d64, gtd.double(), float(d["ln"]), float(d["ls"]),
                          float(d["ld"]), float(d["gamma"]))
    loss.backward()
    assert abs(float(loss) - float(d[f"{tag}_loss"])) < 2e-6
    assert np.allclose(n64.grad.numpy(), d[f"{tag}_dnorm"], atol=1e-8, rtol=2e-4)
    assert np.allclose(d64.grad.numpy(), d[f"{tag}_ddepth"], atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["s", "m"])
def test_hip_geom_losses_match_reference_golden(lib_built, tag):
    from texgs.losses import geom_losses
    d, norm, gtn, gti, mask, depth, gtd = _gload(tag)
    dev = torch.device("cuda:0")
    n = norm.to(dev).requires_grad_(True)
    z = depth.to(dev).requires_grad_(True)
    loss = geom_losses(n, gtn.to(dev), gti.to(dev), mask.to(dev), z, gtd.to(dev), float(d["ln"]), float(d["ls"]),
                       float(d["gamma"]), float(d["ld"]))
    loss.backward()
    assert abs(float(loss) - float(d[f"{tag}_loss"])) < 3e-6
    gn = d[f"{tag}_dnorm"]
    assert float(np.abs(n.grad.cpu().numpy() - gn).max()) < 1e-3 * float(np.abs(gn).max())
    assert np.allclose(z.grad.cpu().numpy(), d[f"{tag}_ddepth"], atol=1e-9)
    # each term alone (a zero lambda skips the term and its pointers)
    only = geom_losses(norm=n.detach(), gt_image=gti.to(dev), mask=mask.to(dev), lambda_smooth=1.0, gamma=float(d["gamma"]))
    assert abs(float(only) - float(d[f"{tag}_Lnsm"])) < 3e-6
    only = geom_losses(norm=n.detach(), gt_norm=gtn.to(dev), mask=mask.to(dev), lambda_norm=1.0)
    assert abs(float(only) - float(d[f"{tag}_Lnorm"])) < 3e-6


@pytest.mark.gpu
def test_hip_geom_losses_full_size_into_rasterizer_backward(lib_built):
    """800x800: HIP vs the float64 restatement, and the produced dL/dnorm flows into the rasterizer's backward."""
    from texgs.losses import geom_losses
    g = torch.Generator().manual_seed(6)
    H = W = 800
    norm = torch.randn(3, H, W, generator=g) * 0.5
    gtn = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0)
    gti = torch.rand(3, H, W, generator=g)
    mask = (torch.rand(1, H, W, generator=g) > 0.2).float()
    dev = torch.device("cuda:0")
    n = norm.to(dev).requires_grad_(True)
    loss = geom_losses(norm=n, gt_norm=gtn.to(dev), gt_image=gti.to(dev), mask=mask.to(dev), lambda_norm=0.1, lambda_smooth=0.5)
    loss.backward()
    n64 = norm.double().requires_grad_(True)
    ref = LO.geom_losses(n64, gtn.double(), gti.double(), mask.double(), None, None, 0.1, 0.5, 0.0)
    ref.backward()
    assert abs(float(loss) - float(ref)) < 5e-6
    assert float((n.grad.cpu().double() - n64.grad).abs().max()) < 1e-3 * float(n64.grad.abs().max())


# ---- pseudo-normal from depth + norm_reg_loss (losses/norm_reg_loss.py:16-78), fixture generated from the reference itself
ND = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_from_depth.npz")


def _nload(tag):
    d = np.load(ND)
    t = lambda k: torch.tensor(d[f"{tag}_{k}"])
    return d, t("depth"), t("wvt"), math.tan(float(d[f"{tag}_fov"][0]) * 0.5), math.tan(float(d[f"{tag}_fov"][1]) * 0.5)


def _check_norm_mask(norm2, mask, d, tag, tol):
    """The normal is a ratio of differences of nearby back-projected points (cancellation: ~1e-4 relative in fp32), and the
    mask compares such differences with a threshold: both are compared where the reference's own mask decision has margin."""
    gm, gn = d[f"{tag}_mask"], d[f"{tag}_norm2"]
    mism = float((mask != gm).mean())
    assert mism < 0.01, mism
    both = (mask == gm)
    err = float(np.abs(norm2 - gn)[np.broadcast_to(both, gn.shape)].max())
    assert err < tol, err
    return mism, err


@pytest.mark.parametrize("tag", ["a", "b"])
def test_norm_from_depth_restatement_matches_reference(tag):
    d, depth, wvt, tx, ty = _nload(tag)
    norm2, mask = LO.norm_from_depth(depth, wvt, tx, ty)
    _check_norm_mask(norm2.numpy(), mask.numpy(), d, tag, 2e-4)
    pred = torch.tensor(d[f"{tag}_pred"]).requires_grad_(True)
    loss = LO.norm_reg_loss(pred, depth, wvt, tx, ty, torch.tensor(d[f"{tag}_gt_alpha"]))
    loss.backward()
    assert abs(float(loss) - float(d[f"{tag}_loss"])) < 2e-5
    assert float(np.abs(pred.grad.numpy() - d[f"{tag}_dpred"]).max()) < 2e-3 * float(np.abs(d[f"{tag}_dpred"]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_hip_norm_from_depth_matches_reference_golden(lib_built, tag):
    from texgs.losses import norm_from_depth, norm_reg_loss
    import helpers as Hh
    d, depth, wvt, tx, ty = _nload(tag)
    dev = torch.device("cuda:0")
    norm2, mask = norm_from_depth(depth.to(dev), wvt, tx, ty)
    mism, err = _check_norm_mask(norm2.cpu().numpy(), mask.cpu().numpy(), d, tag, 1e-3)
    pred = torch.tensor(d[f"{tag}_pred"]).to(dev).requires_grad_(True)
    loss = norm_reg_loss(pred, depth.to(dev), wvt, tx, ty, torch.tensor(d[f"{tag}_gt_alpha"]).to(dev))
    loss.backward()
    gerr = float(np.abs(pred.grad.cpu().numpy() - d[f"{tag}_dpred"]).max()) / float(np.abs(d[f"{tag}_dpred"]).max())
    Hh.report(f"norm_from_depth/{tag}_vs_reference_golden", mask_mismatch_frac=mism, normal_max_abs=err,
              loss_abs=abs(float(loss) - float(d[f"{tag}_loss"])), grad_rel_max=gerr)
    assert abs(float(loss) - float(d[f"{tag}_loss"])) < 5e-5
    assert gerr < 5e-3


@pytest.mark.gpu
def test_hip_norm_from_depth_full_size_vs_restatement(lib_built):
    """800x800 depth from the rasterizer itself; float64 restatement as the checker."""
    from texgs import synth
    from texgs.losses import norm_from_depth
    import helpers as Hh
    dev = torch.device("cuda:0")
    scene = synth.make_scene(30000, 128, seed=3, scale_mean=0.02)
    cam = synth.fibonacci_cameras(4, 800, 800)[1]
    out = Hh.hip_run(scene, cam, 2, torch.zeros(3))[0]
    depth = out[1].detach()
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    norm2, mask = norm_from_depth(depth, cam.world_view_transform, tx, ty)
    rn, rm = LO.norm_from_depth(depth.cpu().double(), cam.world_view_transform.double(), tx, ty)
    mism = float((mask.cpu().double() != rm).double().mean())
    both = (mask.cpu().double() == rm) & (rm > 0)
    e = (norm2.cpu().double() - rn).abs().amax(dim=0, keepdim=True)[both]
    # differences of nearby back-projected points cancel in fp32 (eps * |xyz| / step ~ 1e-4 relative); where the surface step
    # itself is tiny the direction is ill-conditioned, hence a quantile next to the maximum
    p999 = float(torch.quantile(e, 0.999)) if e.numel() else 0.0
    Hh.report("norm_from_depth/800x800_vs_fp64_restatement", mask_mismatch_frac=mism, normal_abs_p999_valid=p999,
              normal_abs_max_valid=float(e.max()) if e.numel() else 0.0, valid_frac=float(rm.mean()))
    assert mism < 0.01 and p999 < 1e-2


# ---- host-side terms next to the operator, pinned to the reference's own functions (tests/golden/host_terms.npz)
HT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_terms.npz")


def test_zero_one_loss_matches_reference():
    from texgs.losses import zero_one_loss
    d = np.load(HT)
    v = torch.tensor(d["zo_value"]).requires_grad_(True)
    loss = zero_one_loss(v)
    loss.backward()
    assert abs(float(loss) - float(d["zo_loss"])) < 1e-6
    assert np.allclose(v.grad.numpy(), d["zo_grad"], rtol=1e-6, atol=1e-9)


def test_depth2world_matches_reference():
    from texgs.losses import depth2world
    d = np.load(HT)
    xyz = depth2world(torch.tensor(d["d2w_depth"]), torch.tensor(d["d2w_full_proj"]), float(d["d2w_zfar"]), float(d["d2w_znear"]))
    assert xyz.shape == (17, 23, 3)
    # the formula against the reference's, both in float64: the fp32 4x4 inverse (cond ~1.5e3) rounds differently on different
    # hosts' BLAS paths (5.4e-5 .. 8.8e-5 from the exact points, the reference's own fp32 result included), so fp32 is held to the
    # exact points instead of to another host's rounding
    xyz64 = depth2world(torch.tensor(d["d2w_depth"]).double(), torch.tensor(d["d2w_full_proj"]).double(), float(d["d2w_zfar"]),
                        float(d["d2w_znear"]))
    assert float(np.abs(xyz64.numpy() - d["d2w_xyz64"]).max()) < 1e-6
    assert float(np.abs(xyz.double().numpy() - d["d2w_xyz64"]).max()) < 2e-4
    # and it inverts the projection: points at view depth d along each pixel's ray project back onto the pixel grid
    full = torch.tensor(d["d2w_full_proj"]).double()
    p = torch.cat([xyz64.reshape(-1, 3), torch.ones(17 * 23, 1, dtype=torch.float64)], dim=1) @ full
    ndc = p[:, :2] / p[:, 3:4]
    gx = ((torch.arange(23, dtype=torch.float64) * 2 + 1) / 23 - 1).repeat(17)
    gy = ((torch.arange(17, dtype=torch.float64) * 2 + 1) / 17 - 1).repeat_interleave(23)
    assert float((ndc[:, 0] - gx).abs().max()) < 1e-4 and float((ndc[:, 1] - gy).abs().max()) < 1e-4
    assert float((p[:, 3] - torch.tensor(d["d2w_depth"]).double().reshape(-1)).abs().max()) < 1e-4
