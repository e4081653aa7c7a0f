"""Generate tests/golden/*.npz.  Runs ONLY in the build container (needs /root/reference); the fixtures (arrays,
no source) travel to the GPU box, the reference does not.

  cameras.npz  utils/graphics.py getWorld2View2 / getProjectionMatrix composed exactly as utils/cameras.py:62-65
               (without the .cuda() calls) -> world_view_transform, full_proj_transform, camera_center
  sh.npz       utils/sh.py eval_sh, degrees 0..3, random coefficients and unit directions
  cube.npz     models/modules/NVDIFFREC/util.py cube_to_dir for all six faces on a texel-centre grid
               (the module imports nvdiffrast and imageio at top level, absent here; throw-away empty module objects are
               registered under those names for the import only -- cube_to_dir itself is pure torch)
  losses.npz   losses/pixelwise_loss.py l1_loss and losses/ssim_loss.py ssim_loss on small random images
  loss_frontend.npz  (1-l)*l1 + l*(1-ssim) + la*l1(alpha) with those functions AND their autograd gradients: the
               fused HIP loss front-end (texgs.losses) is pinned against the reference itself
  geom_losses.npz  losses/norm_reg_loss.py norm_loss, losses/smooth_loss.py smooth_loss and losses/pixelwise_loss.py l1_loss
               combined as models/texture_gaussian3d.py:347-368 combines them (lambda_norm 0.1, lambda_norm_smooth 0.5 of
               configs/texture_gaussian3d.yaml, plus a depth term), values AND autograd gradients w.r.t. norm / depth
  loss_edges.npz  the same reference functions (l1_loss, ssim_loss, norm_loss, smooth_loss) and their autograd at the shapes and
               values where the fused kernels take other paths: images smaller than the 11-tap SSIM window (1x1, 1x9, 9x1, 5x7),
               one partial-tile case (17x31), exact ties (img == gt, alpha == gt_alpha, depth == gt_depth, piecewise-constant
               normals with a zero region), img = gt + 1e-3 noise, a fractional mask, gamma 0.1 and 0.01; every term alone with
               its own gradient (dimg for lambda_dssim 0 / 1 / 0.2)
  norm_from_depth.npz  losses/norm_reg_loss.py norm_from_depth (pseudo-normal + mask of a depth map) and norm_reg_loss with its
               autograd gradient w.r.t. the predicted normal, two cameras from utils/graphics.py getWorld2View2
  host_terms.npz  losses/zero_one_loss.py zero_one_loss (value + autograd gradient, both clamps hit) and
               TextureGaussian3D.depth2world (models/texture_gaussian3d.py:299-309) on a random depth map, in fp32 and float64
  uvnet.npz    models/modules/uv_net.py UVNet with models/modules/utils.py build_nn_network (the `use_tcnn: False` path; utils.py
               imports tinycudann at top level, so the class / function definitions are taken from the two sources with `ast`
               and RUN): weights, embedding, 64 points, uvs, and the Jacobian exactly as
               models/texture_gaussian3d.py:216-227 computes it (autograd.functional.jacobian of the column sums)
  texture_io.npz  models/texture_gaussian3d.py rgb2sh0 / sh02rgb / cube_map / change_texture(modes -1..3): the module
               itself cannot be imported here (cv2, tinycudann, nvdiffrast), so the four function definitions are taken
               from its source with `ast` at generation time and RUN (nothing of them is stored); input = a 12-px-per-face
               downsample of assets/textures/mosaic.png and a random SH-DC texture
  ckpt_stage3.pth  a stage-3 checkpoint FILE as the reference writes it: TextureGaussian3D.setup_optim and .state_dict
               (models/texture_gaussian3d.py:99-172; method definitions taken from the source with `ast` and RUN on a stand-in
               object) + torch.save((state_dict, iteration)) of train.py:181-184.  40 Gaussians, R = 4; nn.Parameter entries,
               three Adam states after one step, the ChainedScheduler state; uv_net / inv_uv_net hold their weights the way
               the shipped configs do (`use_tcnn: True`: one flat `params` tensor per tiny-cuda-nn network -- stand-in
               modules with that one parameter, tinycudann itself is not installable here).  ckpt_stage3_expect.npz: uvs of
               16 points by plain float64 torch from the matrices that were packed into those flat tensors.
  op_small.npz the operator itself on a tiny seeded scene, as computed by oracle/texgs_torch.py in float64
               (regression pin of the oracle; the reference holds no vector for the operator: parity unpinned)
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [ROOT, os.path.join(ROOT, "texture-gs_amd"), os.path.join(ROOT, "tests")]


def cameras():
    sys.path.insert(0, REF)
    from utils.graphics import getWorld2View2, getProjectionMatrix
    rng = np.random.RandomState(0)
    out = {}
    for i in range(4):
        # random rotation (QR) and translation; (R, T) as utils/cameras.py:22-26 takes them
        q, _ = np.linalg.qr(rng.randn(3, 3))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        T = rng.randn(3) * 2.0
        fovx, fovy = 0.4 + 0.3 * i, 0.5 + 0.2 * i
        wvt = torch.tensor(getWorld2View2(q, T, np.array([0.0, 0.0, 0.0]), 1.0)).transpose(0, 1)
        proj = getProjectionMatrix(znear=0.01, zfar=100.0, fovX=fovx, fovY=fovy).transpose(0, 1)
        full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0)
        center = wvt.inverse()[3, :3]
        out[f"R{i}"] = q; out[f"T{i}"] = T; out[f"fov{i}"] = np.array([fovx, fovy])
        out[f"wvt{i}"] = wvt.numpy(); out[f"proj{i}"] = proj.numpy(); out[f"full{i}"] = full.numpy()
        out[f"center{i}"] = center.numpy()
    np.savez(os.path.join(HERE, "cameras.npz"), **out)


def sh():
    sys.path.insert(0, REF)
    from utils.sh import eval_sh, C0
    g = torch.Generator().manual_seed(3)
    dirs = torch.randn(64, 3, generator=g, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    coef = torch.randn(64, 3, 16, generator=g, dtype=torch.float64)      # [..., C, (deg+1)^2]
    out = {"dirs": dirs.numpy(), "coef": coef.numpy(), "C0": np.array(C0)}
    for deg in range(4):
        out[f"deg{deg}"] = eval_sh(deg, coef, dirs).numpy()
    np.savez(os.path.join(HERE, "sh.npz"), **out)


def cube():
    sys.path.insert(0, REF)
    for name in ("nvdiffrast", "nvdiffrast.torch", "imageio"):   # import-only placeholders, see module docstring
        sys.modules.setdefault(name, types.ModuleType(name))
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvdiffrec_util", os.path.join(REF, "models/modules/NVDIFFREC/util.py"))
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    Rr = 8
    c = (torch.arange(Rr, dtype=torch.float64) + 0.5) / Rr * 2.0 - 1.0     # texel centres in [-1,1]
    gy, gx = torch.meshgrid(c, c, indexing="ij")
    dirs = torch.stack([util.cube_to_dir(s, gx, gy) for s in range(6)], 0)   # [6,R,R,3]; x <-> column, y <-> row
    np.savez(os.path.join(HERE, "cube.npz"), dirs=dirs.numpy(), R=np.array(Rr))


def losses():
    sys.path.insert(0, REF)
    from losses.pixelwise_loss import l1_loss
    from losses.ssim_loss import ssim_loss
    g = torch.Generator().manual_seed(9)
    a = torch.rand(3, 24, 20, generator=g)
    b = torch.rand(3, 24, 20, generator=g)
    np.savez(os.path.join(HERE, "losses.npz"), a=a.numpy(), b=b.numpy(), l1=float(l1_loss(a, b)),
             ssim=float(ssim_loss(a, b)))
    # the loss front-end of models/texture_gaussian3d.py:333-345 with the reference's own functions and autograd
    out = {}
    for tag, (H, W) in {"s": (40, 52), "m": (96, 80)}.items():
        img = torch.rand(3, H, W, generator=g).requires_grad_(True)
        gt = (torch.rand(3, H, W, generator=g) * 0.5 + 0.25 * img.detach()).clamp(0, 1)
        alpha = torch.rand(1, H, W, generator=g).requires_grad_(True)
        gta = (torch.rand(1, H, W, generator=g) > 0.4).float()
        lam, la = 0.2, 0.1                              # configs/texture_gaussian3d.yaml lambda_dssim / lambda_alpha
        Ll1 = l1_loss(img, gt)
        Lssim = 1.0 - ssim_loss(img, gt)
        loss = (1.0 - lam) * Ll1 + lam * Lssim + la * l1_loss(alpha, gta)
        loss.backward()
        out.update({f"{tag}_img": img.detach().numpy(), f"{tag}_gt": gt.numpy(), f"{tag}_alpha": alpha.detach().numpy(),
                    f"{tag}_gta": gta.numpy(), f"{tag}_loss": float(loss), f"{tag}_l1": float(Ll1), f"{tag}_ssim": float(1.0 - Lssim),
                    f"{tag}_dimg": img.grad.numpy(), f"{tag}_dalpha": alpha.grad.numpy(), "lam": lam, "la": la})
    np.savez_compressed(os.path.join(HERE, "loss_frontend.npz"), **out)


def geom_losses():
    sys.path.insert(0, REF)
    from losses.pixelwise_loss import l1_loss
    from losses.norm_reg_loss import norm_loss
    from losses.smooth_loss import smooth_loss
    g = torch.Generator().manual_seed(21)
    out = {}
    for tag, (H, W) in {"s": (21, 27), "m": (48, 40)}.items():
        norm = torch.randn(3, H, W, generator=g)
        norm = (norm / norm.norm(dim=0, keepdim=True) * (0.3 + 0.7 * torch.rand(1, H, W, generator=g))).requires_grad_(True)
        gtn = torch.randn(3, H, W, generator=g)
        gtn = gtn / gtn.norm(dim=0, keepdim=True)
        # piecewise-smooth image so the bilateral weights span (0, 1]
        gti = (torch.rand(3, H // 6 + 1, W // 6 + 1, generator=g).repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :H, :W]
               + 0.05 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
        mask = (torch.rand(1, H, W, generator=g) > 0.25).float()
        depth = (3.0 + torch.rand(1, H, W, generator=g)).requires_grad_(True)
        gtd = 3.0 + torch.rand(1, H, W, generator=g)
        ln, ls, ld = 0.1, 0.5, 0.3
        Lnorm = norm_loss(norm, gtn, mask)
        Lnsm = smooth_loss(gti, norm, mask)
        Ld = l1_loss(depth, gtd)
        loss = ln * Lnorm + ls * Lnsm + ld * Ld
        loss.backward()
        out.update({f"{tag}_norm": norm.detach().numpy(), f"{tag}_gtn": gtn.numpy(), f"{tag}_gti": gti.numpy(),
                    f"{tag}_mask": mask.numpy(), f"{tag}_depth": depth.detach().numpy(), f"{tag}_gtd": gtd.numpy(),
                    f"{tag}_loss": float(loss), f"{tag}_Lnorm": float(Lnorm), f"{tag}_Lnsm": float(Lnsm), f"{tag}_Ld": float(Ld),
                    f"{tag}_dnorm": norm.grad.numpy(), f"{tag}_ddepth": depth.grad.numpy()})
        # mask = None variant of the smoothness term is not reachable in the reference (mask.float() on None): skipped
    out.update(ln=0.1, ls=0.5, ld=0.3, gamma=0.1)
    np.savez_compressed(os.path.join(HERE, "geom_losses.npz"), **out)


LOSS_EDGE_RGB = {"1x1": "noise", "1x9": "noise", "9x1": "noise", "5x7": "ties", "17x31": "near"}
LOSS_EDGE_GEOM = ["1x1", "1x9", "9x1", "2x2", "17x15"]


def loss_edges():
    """The reference's loss functions in float32, as the reference runs them, at the edge shapes and values listed in the module
    docstring.  Arrays only; every term separately with its own autograd gradient."""
    sys.path.insert(0, REF)
    from losses.pixelwise_loss import l1_loss
    from losses.ssim_loss import ssim_loss
    from losses.norm_reg_loss import norm_loss
    from losses.smooth_loss import smooth_loss
    g = torch.Generator().manual_seed(33)
    f32, f64 = (lambda t: t.detach().numpy().astype(np.float32)), (lambda v: np.array(float(v.detach()), dtype=np.float64))
    out = {}
    for shp, regime in LOSS_EDGE_RGB.items():
        H, W = (int(v) for v in shp.split("x"))
        gt = torch.rand(3, H, W, generator=g)
        if regime == "near":
            img = gt + 1e-3 * torch.randn(3, H, W, generator=g)
        else:
            img = torch.rand(3, H, W, generator=g)
            if regime == "ties":
                img[:, :, :W // 2] = gt[:, :, :W // 2]
        gta = (torch.rand(1, H, W, generator=g) > 0.4).float()
        alpha = torch.rand(1, H, W, generator=g)
        if H * W > 1:
            alpha[:, :(H + 1) // 2, :(W + 1) // 2] = gta[:, :(H + 1) // 2, :(W + 1) // 2]      # saturated alpha: exact ties
        t = f"rgb{shp}"
        out.update({f"{t}_img": f32(img), f"{t}_gt": f32(gt), f"{t}_alpha": f32(alpha), f"{t}_gta": f32(gta)})
        out.update({f"{t}_Ll1": f64(l1_loss(img, gt)), f"{t}_ssim": f64(ssim_loss(img, gt))})
        for name, lam in (("l0", 0.0), ("l1", 1.0), ("l02", 0.2)):
            i = img.clone().requires_grad_(True)
            ((1.0 - lam) * l1_loss(i, gt) + lam * (1.0 - ssim_loss(i, gt))).backward()
            out[f"{t}_dimg_{name}"] = f32(i.grad)
        a = alpha.clone().requires_grad_(True)
        La = l1_loss(a, gta)
        La.backward()
        out.update({f"{t}_Lalpha": f64(La), f"{t}_dalpha": f32(a.grad)})
    for shp in LOSS_EDGE_GEOM:
        H, W = (int(v) for v in shp.split("x"))
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        # piecewise-constant normals (3x3 blocks) with a zero region, as a render has on the background: ties in the smoothness term
        norm = (torch.randn(3, H // 3 + 1, W // 3 + 1, generator=g) * 0.5).repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W]
        norm = norm * ((xx + yy) < 2 * (H + W) // 3).float()
        gtn = torch.randn(3, H, W, generator=g)
        gtn = gtn / gtn.norm(dim=0, keepdim=True)
        gti = (torch.rand(3, H // 6 + 1, W // 6 + 1, generator=g).repeat_interleave(6, 1).repeat_interleave(6, 2)[:, :H, :W]
               + 0.05 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
        mask = torch.rand(1, H, W, generator=g) * (torch.rand(1, H, W, generator=g) > 0.25).float()      # fractional, with zeros
        gtd = 3.0 + torch.rand(1, H, W, generator=g)
        depth = 3.0 + torch.rand(1, H, W, generator=g)
        if H * W > 1:
            depth[:, :(H + 1) // 2, :(W + 1) // 2] = gtd[:, :(H + 1) // 2, :(W + 1) // 2]
        t = f"geo{shp}"
        out.update({f"{t}_norm": f32(norm), f"{t}_gtn": f32(gtn), f"{t}_gti": f32(gti), f"{t}_mask": f32(mask),
                    f"{t}_depth": f32(depth), f"{t}_gtd": f32(gtd)})
        n = norm.clone().requires_grad_(True)
        Ln = norm_loss(n, gtn, mask)
        Ln.backward()
        out.update({f"{t}_Lnorm": f64(Ln), f"{t}_dnorm_n": f32(n.grad)})
        for name, gamma in (("g01", 0.1), ("g001", 0.01)):
            n = norm.clone().requires_grad_(True)
            Ls = smooth_loss(gti, n, mask, gamma)
            Ls.backward()
            out.update({f"{t}_Lnsm_{name}": f64(Ls), f"{t}_dnorm_s_{name}": f32(n.grad)})
        d = depth.clone().requires_grad_(True)
        Ld = l1_loss(d, gtd)
        Ld.backward()
        out.update({f"{t}_Ld": f64(Ld), f"{t}_ddepth": f32(d.grad)})
    np.savez_compressed(os.path.join(HERE, "loss_edges.npz"), **out)


def norm_from_depth():
    """losses/norm_reg_loss.py norm_from_depth / norm_reg_loss on a smooth synthetic depth map (a tilted, gently bumpy
    surface with one depth step so that the mask has both values), camera from utils/graphics.py getWorld2View2."""
    sys.path.insert(0, REF)
    from losses.norm_reg_loss import norm_from_depth as ref_nfd, norm_reg_loss as ref_nrl
    from utils.graphics import getWorld2View2
    rng = np.random.RandomState(5)
    g = torch.Generator().manual_seed(5)
    out = {}
    for tag, (H, W, fovx, fovy) in {"a": (40, 52, 0.9, 0.7), "b": (33, 24, 0.5, 0.65)}.items():
        q, _ = np.linalg.qr(rng.randn(3, 3))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        wvt = torch.tensor(getWorld2View2(q, rng.randn(3), np.array([0.0, 0.0, 0.0]), 1.0)).transpose(0, 1)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        depth = 0.35 + 0.002 * xx + 0.001 * yy + 0.004 * torch.sin(0.3 * xx) * torch.cos(0.2 * yy)
        depth[:, W // 2:] += 0.05                                  # a depth discontinuity: mask 0 along it
        depth = (depth + 1e-4 * torch.rand(H, W, generator=g)).reshape(1, H, W)

        class View:
            FoVx, FoVy, world_view_transform = fovx, fovy, wvt
        norm2, mask = ref_nfd(depth, View)
        pred = torch.randn(3, H, W, generator=g)
        pred = (pred / pred.norm(dim=0, keepdim=True)).requires_grad_(True)
        gt_alpha = (torch.rand(1, H, W, generator=g) > 0.2).float()
        loss = ref_nrl(pred, depth, View, gt_alpha)
        loss.backward()
        out.update({f"{tag}_depth": depth.numpy(), f"{tag}_wvt": wvt.numpy(), f"{tag}_fov": np.array([fovx, fovy]),
                    f"{tag}_norm2": norm2.numpy(), f"{tag}_mask": mask.numpy(), f"{tag}_pred": pred.detach().numpy(),
                    f"{tag}_gt_alpha": gt_alpha.numpy(), f"{tag}_loss": float(loss), f"{tag}_dpred": pred.grad.numpy()})
    np.savez_compressed(os.path.join(HERE, "norm_from_depth.npz"), **out)


def host_terms():
    """losses/zero_one_loss.py zero_one_loss (importable) and TextureGaussian3D.depth2world (models/texture_gaussian3d.py:299-309,
    taken from the source with `ast` and RUN: the module itself needs tinycudann / cv2), camera matrices from utils/graphics.py."""
    import ast
    sys.path.insert(0, REF)
    from losses.zero_one_loss import zero_one_loss
    from utils.graphics import getWorld2View2, getProjectionMatrix
    g = torch.Generator().manual_seed(9)
    out = {}
    val = torch.rand(500, 1, generator=g)
    val[:20] = 0.0; val[20:40] = 1.0; val[40:60] = 1e-4                      # both clamps
    v = val.clone().requires_grad_(True)
    loss = zero_one_loss(v)
    loss.backward()
    out.update(zo_value=val.numpy(), zo_loss=float(loss), zo_grad=v.grad.numpy())
    src = open(os.path.join(REF, "models", "texture_gaussian3d.py")).read()
    tree = ast.parse(src)
    funcs = [n for cls in tree.body if isinstance(cls, ast.ClassDef) and cls.name == "TextureGaussian3D"
             for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "depth2world"]
    assert len(funcs) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=funcs, type_ignores=[]), "<reference depth2world>", "exec"), ns)
    rng = np.random.RandomState(3)
    q, _ = np.linalg.qr(rng.randn(3, 3))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    znear, zfar, fovx, fovy = 0.01, 100.0, 0.8, 0.6
    wvt = torch.tensor(getWorld2View2(q, rng.randn(3), np.array([0.0, 0.0, 0.0]), 1.0)).transpose(0, 1)
    proj = getProjectionMatrix(znear=znear, zfar=zfar, fovX=fovx, fovY=fovy).transpose(0, 1)
    full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0)
    depth = 2.0 + torch.rand(17, 23, generator=g)
    xyz = ns["depth2world"](None, depth, full, zfar, znear)
    # the same function in float64: the fp32 result above depends on the host's BLAS path (4x4 inverse, cond ~1.5e3)
    xyz64 = ns["depth2world"](None, depth.double(), full.double(), zfar, znear)
    out.update(d2w_depth=depth.numpy(), d2w_full_proj=full.numpy(), d2w_zfar=zfar, d2w_znear=znear, d2w_xyz=xyz.numpy(),
               d2w_xyz64=xyz64.numpy(),
               d2w_wvt=wvt.numpy(), d2w_fov=np.array([fovx, fovy]))
    np.savez_compressed(os.path.join(HERE, "host_terms.npz"), **out)


def uvnet():
    import ast
    from torch import nn
    import torch.nn.functional as F

    class Cfg(dict):                       # addict.Dict stand-in: attribute access, missing keys falsy
        def __getattr__(self, k):
            v = self.get(k)
            return Cfg(v) if isinstance(v, dict) else v
    ns = {"torch": torch, "nn": nn, "F": F, "np": np}
    tree = ast.parse(open(os.path.join(REF, "models", "modules", "utils.py")).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("build_nn_network",)]
    exec(compile(ast.Module(body=fns, type_ignores=[]), "<utils>", "exec"), ns)
    ns["build_mlp"] = lambda cfg, i, o: ns["build_nn_network"](cfg, i, o)      # the not-use_tcnn branch of build_mlp
    tree = ast.parse(open(os.path.join(REF, "models", "modules", "uv_net.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "UVNet"]
    exec(compile(ast.Module(body=cls, type_ignores=[]), "<uv_net>", "exec"), ns)
    torch.manual_seed(3)
    cfg = Cfg(emb_dim=128, pre_mlp_cfg=dict(use_tcnn=False, n_hidden_layers=1, n_neurons=128),
              mlp_cfg=dict(use_tcnn=False, n_hidden_layers=2, n_neurons=128))
    net = ns["UVNet"](cfg).double()          # float32-initialised weights, evaluated in float64 (exactly representable)
    emb = (torch.randn(128) * 0.3).double()
    g = torch.Generator().manual_seed(4)
    xyz = torch.randn(64, 3, generator=g)
    xyz = (xyz / xyz.norm(dim=1, keepdim=True) * (1 + 0.05 * torch.randn(64, 1, generator=g))).double()
    uv = net(xyz, emb)
    jac = torch.autograd.functional.jacobian(lambda inp: net(inp, emb).float().contiguous().sum(dim=0).double(), xyz)
    J = jac.permute(1, 0, 2).reshape(-1, 9)
    out = {k.replace(".", "__"): v.detach().numpy().astype(np.float32) for k, v in net.state_dict().items()}
    out.update(emb=emb.numpy(), xyz=xyz.numpy(), uvs=uv.detach().numpy(), J=J.detach().numpy())
    np.savez_compressed(os.path.join(HERE, "uvnet.npz"), **out)


def texture_io():
    import ast
    from PIL import Image
    src = open(os.path.join(REF, "models", "texture_gaussian3d.py")).read()
    tree = ast.parse(src)
    want_top = {"rgb2sh0", "sh02rgb"}
    want_methods = {"cube_map", "change_texture"}
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want_top]
    for cls in (n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TextureGaussian3D"):
        funcs += [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want_methods]
    assert {f.name for f in funcs} == want_top | want_methods
    ns = {"torch": torch}
    exec(compile(ast.Module(body=funcs, type_ignores=[]), "<reference functions>", "exec"), ns)

    class Holder:                       # the two methods only touch self._texture
        pass
    g = torch.Generator().manual_seed(5)
    r = 12
    mosaic = np.asarray(Image.open(os.path.join(REF, "assets", "textures", "mosaic.png")).convert("RGB"))
    ys = (np.arange(3 * r) * mosaic.shape[0]) // (3 * r)
    xs = (np.arange(4 * r) * mosaic.shape[1]) // (4 * r)
    cross_u8 = mosaic[ys][:, xs]                                  # nearest-neighbour decimation: just a small data sample
    cross = torch.tensor(cross_u8.astype(np.float32) / 255.0)
    tex0 = torch.randn(6, r, r, 3, generator=g) * 1.5
    out = {"cross_u8": cross_u8, "texture0": tex0.numpy()}
    out["sh02rgb"] = ns["sh02rgb"](tex0).numpy()
    out["rgb2sh0"] = ns["rgb2sh0"](cross).numpy()
    h = Holder(); h._texture = tex0.clone()
    out["cube_map"] = ns["cube_map"](h).numpy()
    for mode in (-1, 0, 1, 2, 3):
        h = Holder(); h._texture = tex0.clone()
        ns["change_texture"](h, cross.clone(), mode=mode)
        out[f"change_texture_m{mode + 1}"] = h._texture.numpy()
    np.savez_compressed(os.path.join(HERE, "texture_io.npz"), **out)


def checkpoint():
    import ast
    from torch import nn
    from texgs.uvnet import pack_tcnn_params, HIDDEN
    sys.path.insert(0, REF)
    from utils.general import get_expon_lr_func                       # importable reference piece (pure python)
    src = open(os.path.join(REF, "models", "texture_gaussian3d.py")).read()
    tree = ast.parse(src)
    meths = [n for cls in tree.body if isinstance(cls, ast.ClassDef) and cls.name == "TextureGaussian3D"
             for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("setup_optim", "state_dict")]
    assert len(meths) == 2
    ns = {"torch": torch, "nn": nn, "get_expon_lr_func": get_expon_lr_func}
    exec(compile(ast.Module(body=meths, type_ignores=[]), "<reference TextureGaussian3D methods>", "exec"), ns)

    class Cfg(dict):
        __getattr__ = dict.get

    class TcnnLike(nn.Module):           # what a tcnn.Network looks like to state_dict(): one flat parameter called `params`
        def __init__(self, flat):
            super().__init__()
            self.params = nn.Parameter(flat.clone())

    g = torch.Generator().manual_seed(9)
    rn = lambda *sh, s=1.0: torch.randn(*sh, generator=g) * s
    pre = [(rn(HIDDEN, 3), rn(HIDDEN, s=0.3)), (rn(HIDDEN, HIDDEN, s=0.1), None)]
    mlp = [(rn(HIDDEN, HIDDEN, s=0.1), None), (rn(HIDDEN, HIDDEN, s=0.1), None), (rn(3, HIDDEN), None)]

    class Net(nn.Module):
        def __init__(self, a, b):
            super().__init__()
            self.pre_mlp, self.mlp = a, b
    uv_net = Net(TcnnLike(pack_tcnn_params(pre, 3, HIDDEN)), TcnnLike(pack_tcnn_params(mlp, HIDDEN, 3)))
    # inv_uv_net: hash-grid encoding + MLP = nn.Sequential(enc, mlp) -> keys pre_mlp.0.params / pre_mlp.1.params
    inv_net = Net(nn.Sequential(TcnnLike(rn(4096, s=0.01)), TcnnLike(rn(32 * 128 + 128 * 128, s=0.1))), TcnnLike(rn(2 * 128 * 128 + 16 * 128, s=0.1)))
    N, R = 40, 4

    class Stub:
        pass
    m = Stub()
    m.max_sh_degree, m.active_sh_degree, m.spatial_lr_scale = 3, 3, 1.7
    m._xyz = nn.Parameter(rn(N, 3)); m._scaling = nn.Parameter(rn(N, 3) - 4.0); m._rotation = nn.Parameter(rn(N, 4))
    m._opacity = nn.Parameter(rn(N, 1)); m._shs = nn.Parameter(rn(N, 15, 3, s=0.1)); m._texture = nn.Parameter(rn(6, R, R, 3))
    m.uv_net, m.inv_uv_net, m.geo_emb = uv_net, inv_net, nn.Embedding(1, 128)
    optim_cfg = Cfg(position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
                    opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, tex_lr=0.0025, uv_net_lr=0.00002, inv_uv_net_lr=0.00002,
                    uv_net_milestones=[10000, 20000], uv_net_gamma=0.1)
    ns["setup_optim"](m, optim_cfg)
    loss = sum((p ** 2).sum() for p in (m._xyz, m._scaling, m._rotation, m._opacity, m._shs, m._texture)) \
        + sum((p ** 2).sum() for net in (uv_net, inv_net, m.geo_emb) for p in net.parameters())
    loss.backward()
    for o in (m.optimizer, m.optimizer_uv, m.optimizer_tex):
        o.step()
    m.scheduler_uv.step()
    sd = ns["state_dict"](m)
    torch.save((sd, 40000), os.path.join(HERE, "ckpt_stage3.pth"))           # train.py:181-184
    # what the flat uv_net state evaluates to (plain float64 torch on the matrices AFTER the optimizer step: unpack by hand here)
    def mats(flat, n_in, n_out, hidden):
        pin, pout = -(-n_in // 16) * 16, -(-n_out // 16) * 16
        shapes = [(128, pin)] + [(128, 128)] * (hidden - 1) + [(pout, 128)]
        out, off = [], 0
        for a, b in shapes:
            out.append(flat[off:off + a * b].reshape(a, b).double()); off += a * b
        return out
    p1, p2 = mats(uv_net.pre_mlp.params.detach(), 3, 128, 1)
    q1, q2, q3 = mats(uv_net.mlp.params.detach(), 128, 3, 2)
    xyz = torch.randn(16, 3, generator=g).double()
    emb = m.geo_emb.weight.detach()[0].double()
    x16 = torch.cat([xyz, torch.ones(16, 13, dtype=torch.float64)], 1)            # identity encoding padded with ones
    h = torch.relu(x16 @ p1.t()); a = torch.relu(h @ p2.t() + emb)
    h = torch.relu(torch.relu(a @ q1.t()) @ q2.t()); o = (h @ q3.t())[:, :3]
    np.savez_compressed(os.path.join(HERE, "ckpt_stage3_expect.npz"), xyz=xyz.numpy(), uvs=torch.nn.functional.normalize(o, dim=-1).numpy(),
                        xyz_param=m._xyz.detach().numpy(), texture=m._texture.detach().numpy())


def op_small():
    from texgs import synth
    import helpers as Hh
    scene = synth.make_scene(200, 16, seed=11, scale_mean=0.06)
    cam = synth.fibonacci_cameras(4, 64, 48)[1]
    bg = torch.tensor([0.2, 0.1, 0.3])
    target, nhat = synth.make_targets(48, 64, seed=2)
    ref, dbg, grads = Hh.oracle_run(scene, cam, 2, bg, with_grad=True, target=target, nhat=nhat, depth_weight=0.05)
    out = dict(image=ref[0].detach().numpy(), depth=ref[1].detach().numpy(), norm=ref[2].detach().numpy(),
               alpha=ref[3].detach().numpy(), radii=ref[4].numpy(), n_contrib=dbg["n_contrib"].numpy(),
               ambiguity=dbg["ambiguity"].numpy(), point_list=dbg["binning"]["point_list"].numpy(),
               ranges=dbg["binning"]["ranges"].numpy(), tiles=dbg["pre"]["tiles"].numpy())
    for k, v in grads.items():
        out["grad_" + k] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "op_small.npz"), **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["cameras", "sh", "cube", "losses", "geom_losses", "loss_edges", "norm_from_depth", "host_terms", "uvnet", "texture_io", "checkpoint", "op_small"]
    for name in which:
        globals()[name]()
    print("golden fixtures written to", HERE)
