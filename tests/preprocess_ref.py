"""TEST INFRASTRUCTURE ONLY -- K1 (k_preprocess_fwd) and K8 (k_preprocess_bwd) on their own against float64.

* record64: the dict of oracle.texgs_torch.preprocess as the 24 R_* slots of csrc/common.h.
* moments_from_pairs / pair_loss: a few synthetic (pixel, Gaussian) pairs per Gaussian with random upstream values, summed into
  K7's accumulator rows (the M_* slots of common.h), and the loss those pairs define, written from the blend formulas.
* cotangent_from_moments: M row -> gradient of the record fields, derived HERE from the definitions in the common.h comment
  (not from K8's code); test_preprocess_host.py holds it to autograd of pair_loss at 1e-10.
* scene builders, one per regime; each asserts its own floor on the count and that every discrete decision of K1 sits clear of its
  threshold in float64 (offending Gaussians are dropped while building, never excused while comparing).
The float64 gradient of <cotangent, record64(inputs)> with respect to the inputs is the reference for K8."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import helpers as Hh
from oracle import texgs_torch as O
from texgs import synth

F64 = torch.float64
W, H = 136, 88                     # neither side a multiple of 16
REC, ACC = 24, 32
R_XY, R_CONIC, R_OP, R_G2, R_GM, R_PHI, R_VD, R_DEPTH, R_N = 0, 2, 5, 6, 8, 14, 17, 20, 21
M_P, M_DEN, M_DN, M_PHI, M_VD, M_DEPTH, M_N = 0, 6, 9, 18, 21, 24, 25
FIELDS = {"xy": (0, 2), "conic": (2, 5), "opacity": (5, 6), "g": (6, 8), "G": (8, 14), "phi": (14, 17), "viewdep": (17, 20),
          "depth": (20, 21), "normal": (21, 24)}
ACC_BITS = {"means3D": 1, "means2D": 2, "shs": 4, "opacities": 8, "scales": 16, "rotations": 32, "uvs": 64, "color_offset": 128,
            "cov3D": 256}
GAP = 1e-4                         # relative distance every discrete decision keeps from its threshold
FLOOR = 8.0 * 2.0 ** -24           # bar for outputs the fp32 restatement passes through exactly: a handful of fp32 roundings
WELL, SHIPPED = 1e-4, 2e-3         # what the fp32 C oracle itself must stay below (well-conditioned regimes / "shipped shape")
INPUTS = {"textured": ["means3D", "means2D", "shs", "opacities", "scales", "rotations", "uvs"],
          "coff": ["means3D", "means2D", "shs", "opacities", "scales", "rotations", "color_offset"],
          "cov": ["means3D", "means2D", "shs", "opacities", "color_offset", "cov3D"]}


class Case:
    """One scene of one regime: `scene` (float32 tensors, the attributes texgs_ref.RefRun reads), the camera, the frame's SH degree
    and scale modifier, boolean masks [N] of the property the regime was built for, and the bar its fp32 restatement must meet."""

    def __init__(self, name, flavour, scene, cam, sh_degree, scale_modifier, bar):
        self.name, self.flavour, self.scene, self.cam = name, flavour, scene, cam
        self.sh_degree, self.scale_modifier, self.bar, self.masks = sh_degree, scale_modifier, bar, {}
        self.N = scene.means3D.shape[0]
        self.K = scene.shs.shape[1]

    @property
    def textured(self):
        return self.flavour == "textured"

    def settings(self):
        return Hh.settings_for(self.cam, self.sh_degree, torch.zeros(3), scale_modifier=self.scale_modifier)

    def attr(self, name):
        return getattr(self.scene, "cov3D_precomp" if name == "cov3D" else name, None)


# --------------------------------------------------------------------------------------------------- float64 statement
def leaves64(case, grad=True):
    L = {n: case.attr(n).to(F64).clone().requires_grad_(grad) for n in INPUTS[case.flavour] if n != "means2D"}
    L["means2D"] = torch.zeros(case.N, 3, dtype=F64, requires_grad=grad)
    return L


def run_pre(case, L):
    """oracle.texgs_torch.preprocess on the leaves.  SH rows beyond K count as absent (sh_active): padded with zeros to 15."""
    N, K = case.N, case.K
    shs = torch.cat([L["shs"], torch.zeros(N, 15 - K, 3, dtype=F64)], 1) if K < 15 else L["shs"]
    if case.textured:
        uvs, juv = L["uvs"], case.scene.gradient_uvs.to(F64)
    else:
        uvs, juv = torch.tensor([0.0, 0.0, 1.0], dtype=F64).expand(N, 3), torch.zeros(N, 9, dtype=F64)
    return O.preprocess(L["means3D"], L["means2D"], shs, L["opacities"], L.get("scales"), L.get("rotations"), uvs, juv,
                        case.settings(), F64, color_offset=L.get("color_offset"), cov3D_precomp=L.get("cov3D"))


def record64(pre, textured=True):
    """[N,24] in the R_* layout: xy, conic, opacity, g, G as [c][0..1], phi, viewdep, depth, normal.  Without a texture there is no
    UV plane: g = G = 0 and phi = (0, 0, 1)."""
    N = pre["xy"].shape[0]
    g, G = pre["g"], pre["G"].reshape(N, 6)
    if not textured:
        g, G = torch.zeros_like(g), torch.zeros_like(G)
    return torch.cat([pre["xy"], pre["conic"], pre["opacity"][:, None], g, G, pre["phi"], pre["viewdep"], pre["depth"][:, None],
                      pre["normal"]], 1)


def cotangent_from_moments(M, pre, textured=True):
    """K7's accumulator rows M [N,32] -> dL/d(record) [N,24], float64, record values detached.  From the definitions:
      power = -1/2 ca dx^2 - cb dx dy - 1/2 cc dy^2, dx = xy - pixel, P = dL/dpower:
          dL/dca = -1/2 sum P dx^2, dL/dcb = -sum P dx dy, dL/dcc = -1/2 sum P dy^2,
          dL/dxy = sum P dpower/ddx = -(ca sum P dx + cb sum P dy, cb sum P dx + cc sum P dy)
      alpha = op exp(power): dL/dop = sum dL/dalpha exp(power) = sum P / op         (op = 0: alpha = 0 = P, nothing flows)
      uv = phi + (G dp) / den, den = 1 + g.dp, dp = pixel - xy, dden = dL/dden, dn_c = dL/d(G_c.dp):
          dL/dg_j = sum dden dp_j, dL/dG_cj = sum dn_c dp_j, dL/dphi = sum dL/duv,
          dL/dxy_j += -(g_j sum dden + sum_c G_cj sum dn_c)                          (d dp / d xy = -1)
      viewdep, depth, normal: the sums themselves."""
    rec = record64(pre, textured).detach()
    N = rec.shape[0]
    ca, cb, cc, op = rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5]
    g, G = rec[:, 6:8], rec[:, 8:14].reshape(N, 3, 2)
    sP, sPx, sPy = M[:, M_P], M[:, M_P + 1], M[:, M_P + 2]
    sD = M[:, M_DEN]
    sN = torch.stack([M[:, M_DN], M[:, M_DN + 3], M[:, M_DN + 6]], 1)
    A = torch.zeros(N, REC, dtype=F64)
    A[:, R_XY] = -(ca * sPx + cb * sPy) - (g[:, 0] * sD + (G[:, :, 0] * sN).sum(1))
    A[:, R_XY + 1] = -(cb * sPx + cc * sPy) - (g[:, 1] * sD + (G[:, :, 1] * sN).sum(1))
    A[:, R_CONIC] = -0.5 * M[:, M_P + 3]
    A[:, R_CONIC + 1] = -M[:, M_P + 4]
    A[:, R_CONIC + 2] = -0.5 * M[:, M_P + 5]
    A[:, R_OP] = torch.where(op > 0, sP / torch.where(op > 0, op, torch.ones_like(op)), torch.zeros_like(op))
    A[:, R_G2:R_G2 + 2] = M[:, M_DEN + 1:M_DEN + 3]
    for c in range(3):
        A[:, R_GM + 2 * c:R_GM + 2 * c + 2] = M[:, M_DN + 3 * c + 1:M_DN + 3 * c + 3]
    A[:, R_PHI:R_PHI + 3] = M[:, M_PHI:M_PHI + 3]
    A[:, R_VD:R_VD + 3] = M[:, M_VD:M_VD + 3]
    A[:, R_DEPTH] = M[:, M_DEPTH]
    A[:, R_N:R_N + 3] = M[:, M_N:M_N + 3]
    return A


def cotangent_f32(M32, rec32):
    """The same map in float32 numpy on the fp32 record of the C oracle: what an fp32 implementation computes from the f32 rows."""
    f = np.float32
    M, r = M32.astype(f), rec32.astype(f)
    N = M.shape[0]
    A = np.zeros((N, REC), f)
    ca, cb, cc, op = r[:, 2], r[:, 3], r[:, 4], r[:, 5]
    sN = [M[:, M_DN], M[:, M_DN + 3], M[:, M_DN + 6]]
    for j in range(2):
        uvp = (r[:, R_GM + j] * sN[0] + r[:, R_GM + 2 + j] * sN[1] + r[:, R_GM + 4 + j] * sN[2]) + r[:, R_G2 + j] * M[:, M_DEN]
        A[:, R_XY + j] = -((ca if j == 0 else cc) * M[:, M_P + 1 + j] + cb * M[:, M_P + 2 - j]) - uvp
    A[:, R_CONIC], A[:, R_CONIC + 1], A[:, R_CONIC + 2] = f(-0.5) * M[:, M_P + 3], -M[:, M_P + 4], f(-0.5) * M[:, M_P + 5]
    A[:, R_OP] = np.where(op > 0, M[:, M_P] / np.where(op > 0, op, f(1)), f(0))
    A[:, R_G2:R_G2 + 2] = M[:, M_DEN + 1:M_DEN + 3]
    for c in range(3):
        A[:, R_GM + 2 * c:R_GM + 2 * c + 2] = M[:, M_DN + 3 * c + 1:M_DN + 3 * c + 3]
    A[:, R_PHI:R_PHI + 3], A[:, R_VD:R_VD + 3] = M[:, M_PHI:M_PHI + 3], M[:, M_VD:M_VD + 3]
    A[:, R_DEPTH], A[:, R_N:R_N + 3] = M[:, M_DEPTH], M[:, M_N:M_N + 3]
    return A


def moments_from_pairs(pre, seed, textured=True, npairs=4):
    """`npairs` synthetic pairs per Gaussian: integer pixels within the splat's radius of xy, random upstream values P, dden, dn[3],
    dL/duv[3], dL/dcolour[3], w dL/ddepth, w dL/dnormal[3].  -> (pairs, M float64 [N,32]).  A Gaussian of opacity 0 has alpha = 0,
    so P = dL/dalpha alpha = 0 in every one of its pairs; without a texture K7 sums no UV moments.  Rows of culled Gaussians get
    random numbers: K7 never writes them and K8 must not read them."""
    g = torch.Generator().manual_seed(seed)
    N = pre["xy"].shape[0]
    valid = pre["valid"]
    xy = torch.where(valid[:, None], pre["xy"].detach(), torch.zeros(N, 2, dtype=F64))
    rad = pre["radius"].to(F64).clamp(1.0, 40.0)
    off = (2.0 * torch.rand(N, npairs, 2, generator=g, dtype=F64) - 1.0) * rad[:, None, None] * math.sqrt(0.5)
    pix = torch.round(xy[:, None, :] + off)
    rn = lambda *s: torch.randn(N, npairs, *s, generator=g, dtype=F64)
    p = SimpleNamespace(pix=pix, P=rn(), dden=rn(), dn=rn(3), u=rn(3), v=rn(3), z=rn(), nu=rn(3))
    p.P = p.P * (pre["opacity"].detach() > 0).to(F64)[:, None]
    if not textured:
        p.dden, p.dn, p.u = torch.zeros_like(p.dden), torch.zeros_like(p.dn), torch.zeros_like(p.u)
    dx, dy = xy[:, None, 0] - pix[..., 0], xy[:, None, 1] - pix[..., 1]
    M = torch.zeros(N, ACC, dtype=F64)
    for k, mono in enumerate([torch.ones_like(dx), dx, dy, dx * dx, dx * dy, dy * dy]):
        M[:, M_P + k] = (p.P * mono).sum(1)
    for k, mono in enumerate([torch.ones_like(dx), -dx, -dy]):
        M[:, M_DEN + k] = (p.dden * mono).sum(1)
        for c in range(3):
            M[:, M_DN + 3 * c + k] = (p.dn[..., c] * mono).sum(1)
    M[:, M_PHI:M_PHI + 3], M[:, M_VD:M_VD + 3] = p.u.sum(1), p.v.sum(1)
    M[:, M_DEPTH], M[:, M_N:M_N + 3] = p.z.sum(1), p.nu.sum(1)
    M[~valid] = torch.randn(int((~valid).sum()), ACC, generator=g, dtype=F64)
    return p, M


def pair_loss(pre, p, textured=True):
    """L_pairs = sum_k P (power + log op) + dden (1 + g.dp) + sum_c dn_c (G_c.dp) + u.phi + v.viewdep + z depth + nu.normal over the
    pairs of the visible Gaussians, straight from the blend formulas (pre carries the autograd graph)."""
    v = pre["valid"]
    xy, con, op = pre["xy"][v], pre["conic"][v], pre["opacity"][v]
    pix = p.pix[v]
    dx, dy = xy[:, None, 0] - pix[..., 0], xy[:, None, 1] - pix[..., 1]
    power = -0.5 * con[:, None, 0] * dx * dx - con[:, None, 1] * dx * dy - 0.5 * con[:, None, 2] * dy * dy
    logop = torch.where(op > 0, torch.log(torch.where(op > 0, op, torch.ones_like(op))), torch.zeros_like(op))
    L = (p.P[v] * (power + logop[:, None])).sum()
    if textured:
        dp = torch.stack([-dx, -dy], -1)
        den = 1.0 + (pre["g"][v][:, None, :] * dp).sum(-1)
        num = (pre["G"][v][:, None, :, :] * dp[:, :, None, :]).sum(-1)
        L = L + (p.dden[v] * den).sum() + (p.dn[v] * num).sum() + (p.u[v] * pre["phi"][v][:, None, :]).sum()
    return (L + (p.v[v] * pre["viewdep"][v][:, None, :]).sum() + (p.z[v] * pre["depth"][v][:, None]).sum()
            + (p.nu[v] * pre["normal"][v][:, None, :]).sum())


def grads_of(case, loss_fn):
    """float64 autograd of loss_fn(pre) with respect to every input of the flavour -> {name: [N,...]} (zeros where nothing flows)"""
    L = leaves64(case)
    loss_fn(run_pre(case, L)).backward()
    return {n: (L[n].grad if L[n].grad is not None else torch.zeros_like(L[n])).detach() for n in INPUTS[case.flavour]}


def reference_grads(case, M):
    def loss(pre):
        v = pre["valid"]
        return (cotangent_from_moments(M, pre, case.textured)[v] * record64(pre, case.textured)[v]).sum()
    return grads_of(case, loss)


def row_error(got, ref, rows=None, operand=None):
    """worst row of max|d| / (max|row| + 1e-4 max|all|), no row excluded (`rows`: the rows looked at, e.g. the visible ones).
    `operand`: `ref` is a sum that the code under test forms in fp32 (start values + gradient) and this is its other operand: a sum
    of two fp32 numbers is accurate relative to the larger operand, not to a result that may cancel, so max|operand row| joins the
    row's denominator."""
    g = torch.as_tensor(got).to(F64).reshape(ref.shape[0], -1)
    e = ref.to(F64).reshape(ref.shape[0], -1)
    o = torch.zeros_like(e) if operand is None else torch.as_tensor(operand).to(F64).reshape(e.shape)
    if rows is not None:
        g, e, o = g[rows], e[rows], o[rows]
    if e.numel() == 0:
        return 0.0
    top = float(e.abs().max())
    if top == 0.0:
        return 0.0 if float(g.abs().max()) == 0.0 else float("inf")
    err = (g - e).abs().max(1).values / (e.abs().max(1).values + o.abs().max(1).values + 1e-4 * top)
    return float(err.max()) if bool(torch.isfinite(g).all()) else float("inf")


# --------------------------------------------------------------------------------------------------- decisions
def _tiles_positive(xy, rf):
    gx, gy = (W + O.TILE - 1) // O.TILE, (H + O.TILE - 1) // O.TILE
    t = lambda v, hi: torch.clamp((v / O.TILE).to(torch.int64), 0, hi)
    return ((t(xy[:, 0] + rf + (O.TILE - 1), gx) - t(xy[:, 0] - rf, gx)) * (t(xy[:, 1] + rf + (O.TILE - 1), gy) - t(xy[:, 1] - rf, gy))) > 0


def decision_gaps(case, pre):
    """{decision: relative gap [N]} of the discrete decisions K1 takes, in float64 (inf where the decision is not taken), and `geo`,
    the view-space quantities the masks are made from."""
    s, st = case.scene, case.settings()
    N = case.N
    inf = torch.full((N,), float("inf"), dtype=F64)
    V, cam = st.viewmatrix.to(F64), st.campos.to(F64)
    m = s.means3D.to(F64)
    t = (torch.cat([m, torch.ones(N, 1, dtype=F64)], 1) @ V)[:, :3]
    tz = t[:, 2]
    front = tz > O.NEAR_Z
    tzs = torch.where(front, tz, torch.ones_like(tz))
    limx, limy = O.FRUSTUM_CLAMP * st.tanfovx, O.FRUSTUM_CLAMP * st.tanfovy
    u, v = t[:, 0] / tzs, t[:, 1] / tzs
    gaps = {"near": (tz - O.NEAR_Z).abs() / O.NEAR_Z,
            "clamp_x": torch.where(front, (u.abs() - limx).abs() / limx, inf),
            "clamp_y": torch.where(front, (v.abs() - limy).abs() / limy, inf)}
    con = pre["conic"].detach()
    det = 1.0 / (con[:, 0] * con[:, 2] - con[:, 1] ** 2)
    gaps["det"] = torch.where(front, det / ((con[:, 2] * det) * (con[:, 0] * det)), inf)
    n = pre["normal"].detach()
    d = m - cam[None]
    gaps["normal_sign"] = torch.where(front, (n * d).sum(1).abs() / (n.norm(dim=1) * d.norm(dim=1)), inf)
    if case.flavour == "cov":
        c6 = s.cov3D_precomp.to(F64)
        S = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(N, 3, 3)
        ev = torch.linalg.eigvalsh(S)
        gaps["shortest_axis"] = (ev[:, 1] - ev[:, 0]) / ev[:, 1]
        kmin = torch.full((N,), -1, dtype=torch.int64)
        raw = -n                                                              # (an eigenvector has no sign of its own)
    else:
        sc = torch.sort(s.scales.to(F64), dim=1).values
        gaps["shortest_axis"] = (sc[:, 1] - sc[:, 0]) / sc[:, 1]
        kmin = torch.argmin(s.scales.to(F64), dim=1)
        raw = O.build_rotation(s.rotations.to(F64))[torch.arange(N), :, kmin]
    sdot = ((n @ V[:3, :3]) * t).sum(1)
    lim = O.PLANE_EPS * t.norm(dim=1)
    gaps["plane"] = torch.where(front, (sdot.abs() - lim).abs() / lim, inf) if case.textured else inf
    op = s.opacities.to(F64).reshape(-1)                                     # K1's thr < 0 <=> 255 op e^0.001 > 1 (record only)
    gaps["thr_sign"] = torch.where(op > 0, (255.0 * op * math.exp(1e-3) - 1.0).abs(), inf)
    # visibility = a non-empty tile rectangle: the same answer with the radius one pixel off and the centre 1e-3 px off
    xy = torch.nan_to_num(pre["xy"].detach(), nan=0.0, posinf=1e9, neginf=-1e9)
    rf = (pre["radius_f"].detach().ceil()).clamp(max=1e9)
    base = _tiles_positive(xy, rf)
    same = torch.ones(N, dtype=torch.bool)
    for dr in (-1.0, 1.0):
        for sx in (-1.0, 1.0):
            for sy in (-1.0, 1.0):
                same &= _tiles_positive(xy + 1e-3 * torch.tensor([sx, sy], dtype=F64) * (1.0 + xy.abs()), rf + dr) == base
    gaps["tile_rect"] = torch.where(front & ~same, torch.zeros_like(inf), inf)
    geo = SimpleNamespace(t=t, front=front, clx=front & (u.abs() > limx), cly=front & (v.abs() > limy), kmin=kmin,
                          flip=(raw * d).sum(1) > 0, degen=front & (sdot.abs() <= lim), sdot=sdot)
    return gaps, geo


def clear_of_thresholds(case, pre):
    gaps, geo = decision_gaps(case, pre)
    ok = torch.ones(case.N, dtype=torch.bool)
    for v in gaps.values():
        ok &= v >= GAP
    return ok, gaps, geo


# --------------------------------------------------------------------------------------------------- scenes
def _unit(v):
    return v / v.norm(dim=1, keepdim=True)


def _quat_z_to(n):
    """unit quaternion (w,x,y,z) taking the local z axis to the unit vector n"""
    N = n.shape[0]
    z = torch.tensor([0.0, 0.0, 1.0], dtype=F64).expand(N, 3)
    axis = torch.cross(z, n, dim=1)
    an = axis.norm(dim=1, keepdim=True)
    axis = torch.where(an > 1e-9, axis / an.clamp_min(1e-30), torch.tensor([1.0, 0.0, 0.0], dtype=F64).expand(N, 3))
    ang = torch.acos(n[:, 2:3].clamp(-1, 1))
    return torch.cat([torch.cos(ang / 2), axis * torch.sin(ang / 2)], 1)


def free_camera(eye, target, fovx, fovy):
    """A camera at `eye` looking at `target` (not the origin) with independent fields of view; full_proj_transform from
    synth.projection."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    Rm = np.stack([right, np.cross(fwd, right), fwd], axis=1)
    wvt = torch.tensor(synth.world2view(Rm, -Rm.T @ eye)).transpose(0, 1).contiguous()
    full = (wvt @ synth.projection(0.01, 100.0, fovx, fovy).transpose(0, 1)).contiguous()
    return synth.Cam(H, W, fovx, fovy, wvt, full, wvt.inverse()[3, :3].contiguous())


def default_camera():
    return synth.look_at_camera((0.4, 0.3, 2.0), W, H)


def box_means(g, n):
    return (torch.rand(n, 3, generator=g, dtype=F64) - 0.5) * torch.tensor([6.0, 4.0, 6.0], dtype=F64)


def view_means(g, cam, n, u, v, tz):
    """means whose view-space position is (u tanfovx tz, v tanfovy tz, tz), u / v / tz uniform in the given ranges"""
    r = lambda lo_hi: lo_hi[0] + (lo_hi[1] - lo_hi[0]) * torch.rand(n, generator=g, dtype=F64)
    z = r(tz)
    t = torch.stack([r(u) * math.tan(cam.FoVx / 2) * z, r(v) * math.tan(cam.FoVy / 2) * z, z], 1)
    V = cam.world_view_transform.to(F64)
    return (t - V[3, :3]) @ torch.linalg.inv(V[:3, :3])


def make_inputs(g, means, smin, smax, K=15, third=None, qnorm=None, quats=None):
    n = means.shape[0]
    scales = torch.exp(math.log(smin) + math.log(smax / smin) * torch.rand(n, 3, generator=g, dtype=F64))
    if third is not None:
        scales[:, 2] = third
    q = _unit(torch.randn(n, 4, generator=g, dtype=F64)) if quats is None else quats
    if qnorm is not None:
        q = q * (qnorm[0] + (qnorm[1] - qnorm[0]) * torch.rand(n, 1, generator=g, dtype=F64))
    f = lambda t: t.to(torch.float32).contiguous()
    return SimpleNamespace(means3D=f(means), scales=f(scales), rotations=f(q),
                           opacities=f(0.05 + 0.95 * torch.rand(n, 1, generator=g, dtype=F64)),
                           shs=f(0.2 * torch.randn(n, K, 3, generator=g, dtype=F64)), uvs=f(_unit(torch.randn(n, 3, generator=g, dtype=F64))),
                           gradient_uvs=f(0.5 * torch.randn(n, 9, generator=g, dtype=F64)), texture=torch.zeros(6, 4, 4, 3),
                           color_offset=None, cov3D_precomp=None)


def to_flavour(g, s, flavour):
    """textured -> the untextured surface with a colour offset ("coff"), or that with a precomputed covariance ("cov": three distinct
    axes, the shortest 0.2-0.5 of the next, so that the eigenvector of the smallest eigenvalue is well defined in fp32)"""
    if flavour == "textured":
        return s
    n = s.means3D.shape[0]
    s.texture = s.uvs = s.gradient_uvs = None
    s.color_offset = (0.3 * torch.randn(n, 3, generator=g, dtype=F64)).float()
    if flavour == "cov":
        sc = s.scales.to(F64).clamp_min(0.02)
        srt = torch.sort(sc, dim=1).values
        sc = torch.stack([srt[:, 2], srt[:, 1], srt[:, 1] * (0.2 + 0.3 * torch.rand(n, generator=g, dtype=F64))], 1)
        M = O.build_rotation(_unit(s.rotations.to(F64))) * sc[:, None, :]
        S = M @ M.transpose(1, 2)
        s.cov3D_precomp = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float().contiguous()
        s.scales = s.rotations = None
    return s


def _take(s, idx):
    out = SimpleNamespace(**vars(s))
    for k, v in vars(s).items():
        if k != "texture" and v is not None:
            setattr(out, k, v[idx].contiguous())
    return out


def finish(name, flavour, scene, cam, N, masks_fn, floors, sh_degree=3, scale_modifier=1.0, bar=WELL, min_visible=50):
    """Drop the candidates that sit within GAP of a threshold, keep the first N, make the masks and assert the floors and the gaps."""
    cand = Case(name, flavour, scene, cam, sh_degree, scale_modifier, bar)
    ok, _, _ = clear_of_thresholds(cand, run_pre(cand, leaves64(cand, grad=False)))
    idx = torch.nonzero(ok).reshape(-1)[:N]
    assert idx.numel() == N, (name, "too few clean candidates", int(ok.sum()), N)
    case = Case(name, flavour, _take(scene, idx), cam, sh_degree, scale_modifier, bar)
    pre = run_pre(case, leaves64(case, grad=False))
    ok, gaps, geo = clear_of_thresholds(case, pre)
    assert bool(ok.all()), {k: float(v.min()) for k, v in gaps.items()}
    vis = pre["valid"]
    case.masks = {"visible": vis, "culled": ~vis}
    case.masks.update({k: (m & ~vis if k.startswith("culled_") else m & vis) for k, m in masks_fn(case, pre, geo).items()})
    counts = {k: int(m.sum()) for k, m in case.masks.items()}
    assert counts["visible"] >= min(min_visible, N), (name, counts)
    for k, least in floors.items():
        assert counts[k] >= least, (name, k, counts)
    case.counts = counts
    return case


def _general_masks(case, pre, geo):
    m = {"clamped": geo.clx | geo.cly}
    if case.flavour != "cov":
        m.update({f"kmin{k}": geo.kmin == k for k in range(3)}, flipped=geo.flip, unflipped=~geo.flip)
    return m


def build_general(flavour="textured", n=1500, K=15, sh_degree=3, seed=101, name="general"):
    g = torch.Generator().manual_seed(seed)
    s = to_flavour(g, make_inputs(g, box_means(g, 2 * n), 0.01, 0.3, K=K), flavour)
    floors = {"clamped": 50}
    if flavour != "cov":
        floors.update(kmin0=50, kmin1=50, kmin2=50, flipped=50, unflipped=50)
    return finish(name, flavour, s, default_camera(), n, _general_masks, floors if n >= 1500 else {}, sh_degree=sh_degree)


def build_clamp(flavour="textured"):
    g = torch.Generator().manual_seed(102)
    cam = default_camera()
    s = to_flavour(g, make_inputs(g, view_means(g, cam, 2400, (-1.9, 1.9), (-1.9, 1.9), (0.8, 3.0)), 0.05, 0.5), flavour)
    masks = lambda c, p, geo: {"x_only": geo.clx & ~geo.cly, "y_only": geo.cly & ~geo.clx, "both": geo.clx & geo.cly}
    return finish("clamp", flavour, s, cam, 1200, masks, {"x_only": 50, "y_only": 50, "both": 50})


def build_near_plane(flavour="textured"):
    g = torch.Generator().manual_seed(103)
    cam = default_camera()
    s = to_flavour(g, make_inputs(g, view_means(g, cam, 800, (-0.9, 0.9), (-0.9, 0.9), (0.1, 0.32)), 0.002, 0.02), flavour)

    def masks(c, p, geo):
        tz = geo.t[:, 2]
        return {"band": (tz > 0.2) & (tz <= 0.3), "culled_band": (tz >= 0.1) & (tz < 0.2)}
    case = finish("near_plane", flavour, s, cam, 400, masks, {"band": 20, "culled_band": 20})
    tz = decision_gaps(case, run_pre(case, leaves64(case, grad=False)))[1].t[:, 2]
    assert torch.equal(case.masks["culled_band"], (tz >= 0.1) & (tz < 0.2)), "a Gaussian behind the near plane is visible"
    return case


def build_degenerate(flavour="textured"):
    """Half the Gaussians see their plane edge-on: |n.t| = |sin(theta)| |t| with |sin| <= 0.045 (threshold 0.05); the others 0.06..1."""
    assert flavour == "textured", "the plane guard exists only with a texture"
    g = torch.Generator().manual_seed(104)
    cam = default_camera()
    n = 1200
    means = view_means(g, cam, n, (-0.9, 0.9), (-0.9, 0.9), (0.8, 4.0))
    d = _unit(means - cam.camera_center.to(F64)[None])
    p = _unit(torch.cross(d, torch.randn(n, 3, generator=g, dtype=F64), dim=1))
    r = torch.rand(n, generator=g, dtype=F64)
    sin = torch.where(torch.arange(n) % 2 == 0, 0.045 * (2 * r - 1), (0.06 + 0.94 * r) * torch.where(r > 0.5, 1.0, -1.0))
    normal = torch.sqrt(1 - sin * sin)[:, None] * p + sin[:, None] * d
    spin = 2 * math.pi * torch.rand(n, 1, generator=g, dtype=F64)
    q = synth._quat_mul(_quat_z_to(normal), torch.cat([torch.cos(spin / 2), torch.zeros(n, 2, dtype=F64), torch.sin(spin / 2)], 1))
    s = make_inputs(g, means, 0.02, 0.2, quats=_unit(q))
    s.scales[:, 2] = 0.3 * s.scales[:, :2].min(dim=1).values
    masks = lambda c, pre, geo: {"degenerate": geo.degen, "regular": ~geo.degen}
    return finish("degenerate_plane", flavour, s, cam, 600, masks, {"degenerate": 50, "regular": 50})


def build_shipped(flavour="textured"):
    assert flavour == "textured"
    g = torch.Generator().manual_seed(105)
    s = make_inputs(g, box_means(g, 3000), 0.01, 0.3, third=math.exp(-20.0), qnorm=(0.5, 2.0))
    return finish("shipped_shape", flavour, s, default_camera(), 1500, lambda c, p, geo: {"clamped": geo.clx | geo.cly}, {"clamped": 50},
                  scale_modifier=0.7, bar=SHIPPED)


def build_camera(flavour="textured"):
    g = torch.Generator().manual_seed(106)
    cam = free_camera((1.5, -0.7, 2.2), (0.8, 0.4, -0.5), 0.9, 0.5)
    s = to_flavour(g, make_inputs(g, box_means(g, 3000), 0.01, 0.3), flavour)
    assert abs(math.tan(cam.FoVy / 2) / math.tan(cam.FoVx / 2) - H / W) > 0.1, "fovy must not follow from fovx"
    return finish("camera", flavour, s, cam, 1500, lambda c, p, geo: {"clamped": geo.clx | geo.cly}, {"clamped": 50})


def build_opacity(flavour="textured"):
    g = torch.Generator().manual_seed(107)
    cam = default_camera()
    s = to_flavour(g, make_inputs(g, view_means(g, cam, 1200, (-1.2, 1.2), (-1.2, 1.2), (0.5, 4.0)), 0.01, 0.2), flavour)
    k = torch.arange(1200)
    s.opacities[k % 3 == 0] = 0.0
    small = k % 3 == 1
    s.opacities[small] = (5e-4 * torch.exp(math.log(4.0) * torch.rand(int(small.sum()), 1, generator=g, dtype=F64))).float()

    def masks(c, p, geo):
        op = c.scene.opacities.reshape(-1)
        return {"zero": op == 0, "small": (op > 0) & (op < 2.5e-3)}
    return finish("opacity", flavour, s, cam, 600, masks, {"zero": 50, "small": 50})


def build_sh(K, sh_degree):
    return build_general(n=500, K=K, sh_degree=sh_degree, seed=108, name=f"sh_K{K}_deg{sh_degree}")


def build_size(n):
    """N Gaussians, nearly all in front of the camera (a tenth behind it)"""
    g = torch.Generator().manual_seed(109)
    cam = default_camera()
    means = view_means(g, cam, 2 * n + 8, (-1.0, 1.0), (-1.0, 1.0), (0.5, 4.0))
    if n > 1:
        behind = torch.arange(2 * n + 8) % 10 == 3
        means[behind] = view_means(g, cam, int(behind.sum()), (-1.0, 1.0), (-1.0, 1.0), (-2.0, 0.1))
    return finish(f"size_{n}", "textured", make_inputs(g, means, 0.01, 0.2), cam, n, lambda c, p, geo: {}, {}, min_visible=50)


SH_CASES = [(15, 0), (15, 1), (15, 2), (15, 3), (4, 1), (4, 3)]
SIZES = [1, 255, 256, 257, 513]
BUILDERS = {"general": build_general, "clamp": build_clamp, "near_plane": build_near_plane, "degenerate_plane": build_degenerate,
            "shipped_shape": build_shipped, "camera": build_camera, "opacity": build_opacity}
BUILDERS.update({f"sh_K{K}_deg{d}": functools.partial(lambda flavour, K, d: build_sh(K, d), K=K, d=d) for K, d in SH_CASES})
BUILDERS.update({f"size_{n}": functools.partial(lambda flavour, n: build_size(n), n=n) for n in SIZES})
REGIMES = list(BUILDERS)
FLAVOURED = [(r, f) for f in ("coff", "cov") for r in ("general", "clamp", "near_plane", "camera", "opacity")]     # the two other flavours of K1 / K8
ALL_CASES = [(r, "textured") for r in REGIMES] + FLAVOURED


@functools.lru_cache(maxsize=None)
def prepared(regime, flavour="textured"):
    """The case, its float64 forward, its pairs and moments, and the float64 reference of K8 for the f32-rounded moments -- computed
    once per process, shared by every test, never modified."""
    case = BUILDERS[regime](flavour)
    pre = run_pre(case, leaves64(case, grad=False))
    pairs, M = moments_from_pairs(pre, seed=7 + len(regime), textured=case.textured)
    M32 = M.to(torch.float32)
    return SimpleNamespace(case=case, pre=pre, pairs=pairs, M=M, M32=M32, rec=record64(pre, case.textured),
                           ref=reference_grads(case, M32.to(F64)), visible=pre["valid"])


# --------------------------------------------------------------------------------------------------- recorded figures
import json
import os

PARITY_JSON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "preprocess_parity.json")


def load_parity():
    try:
        with open(PARITY_JSON) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def store_parity(section, figures):
    """Merge {regime: {flavour: {output: figure}}} into `section` of profiles/preprocess_parity.json (three significant digits)."""
    if not figures:
        return
    doc = load_parity()
    sec = doc.setdefault(section, {})
    for regime, by_flavour in figures.items():
        for flavour, by_output in by_flavour.items():
            sec.setdefault(regime, {}).setdefault(flavour, {}).update({k: float(f"{v:.3e}") for k, v in by_output.items()})
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    try:
        if not os.path.exists(PARITY_JSON) or open(PARITY_JSON).read() != text:
            with open(PARITY_JSON, "w") as f:
                f.write(text)
    except OSError:
        pass


def hip_bar(regime, flavour, output):
    """max(4 x the C oracle's recorded figure, 8 * 2^-24): the factor 4 for device division / sqrt / reciprocal differing from host
    libm by a few ulp through the same amplifying chain, the floor for what the C oracle passes through exactly."""
    fig = load_parity()["c_oracle_vs_f64"][regime][flavour][output]
    return max(4.0 * fig, FLOOR)


def other_uv_cotangents(M32):
    """the rows with other values in the slots that become the g / G cotangents (A[R_G2], A[R_GM]): sum dden dp, sum dn_c dp"""
    M = M32.clone()
    for base in (M_DEN, M_DN, M_DN + 3, M_DN + 6):
        M[:, base + 1:base + 3] = 3.0 * M[:, base + 1:base + 3] + 1.0
    return M


def full_matrix_cov_gradient(case, M):
    """cov flavour: dL/dSigma [N,3,3] with Sigma a full (nine-entry) symmetric leaf"""
    L = leaves64(case, grad=False)
    c6 = L["cov3D"]
    N = case.N
    S = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).reshape(N, 3, 3)
    S = S.clone().requires_grad_(True)
    # the forward reads six entries: feed it the mean of the upper and the lower triangle, so that each half of an off-diagonal
    # pair receives its own share of the gradient
    sym = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    low = torch.stack([S[:, 0, 0], S[:, 1, 0], S[:, 2, 0], S[:, 1, 1], S[:, 2, 1], S[:, 2, 2]], 1)
    L["cov3D"] = 0.5 * (sym + low)
    pre = run_pre(case, L)
    v = pre["valid"]
    (cotangent_from_moments(M, pre, False)[v] * record64(pre, False)[v]).sum().backward()
    return S.grad.detach()
