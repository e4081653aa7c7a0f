"""Generate tests/golden/density.npz: stage-1 density control as the REFERENCE computes it, on the CPU.  Runs only where the reference
tree is (like make_golden.py); the fixture holds arrays only.

The methods of `Gaussian3D` (models/gaussian3d.py) and `build_rotation` / `inverse_sigmoid` (utils/general.py) are taken out of the
sources with `ast` and RUN, after three rewrites: the string constant "cuda" becomes "cpu", `Tensor.cuda` is the identity, and the
`torch.normal(mean, std)` of densify_and_split becomes `mean + std * eps` with the standard-normal `eps` recorded (torch.normal's
stream is not part of the contract; the samples are an input of texgs.density).  setup_optim runs with a stub learning-rate
function, and one optimizer.step() makes the Adam moments non-zero.

  sh3_*, sh1_*   densify_and_prune on N = 400: f_rest [N, 15, 3] with max_screen_size = 20, f_rest [N, 3, 3] without
  prune_*        one opacity_prune (N = 100)
  reset_*        one reset_opacity and one reset_min_scale (N = 100)
  stats_*        two rounds of optimize_step's statistics lines (:431-432) with seeded grad and radii

f_dc, f_rest and every gradient are drawn from a few dozen levels so that the file compresses (they are only ever copied); positions,
scales, rotations and opacities are continuous.  The generator asserts what the fixture is for and fails when a seed misses it."""
import ast
import os
import sys

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (where the reference tree is)
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}
MARGIN = 1e-4
REC = {}


class _Rewrite(ast.NodeTransformer):
    def __init__(self):
        self.fn = []

    def visit_FunctionDef(self, node):
        for a in node.args.args + node.args.kwonlyargs:      # (annotations name classes of modules that are not imported here)
            a.annotation = None
        self.fn.append(node.name)
        self.generic_visit(node)
        self.fn.pop()
        return node

    def visit_Constant(self, node):
        return ast.copy_location(ast.Constant("cpu"), node) if node.value == "cuda" else node

    def visit_Call(self, node):
        self.generic_visit(node)
        f = node.func
        if self.fn and self.fn[-1] == "densify_and_split" and isinstance(f, ast.Attribute) and f.attr == "normal" \
                and isinstance(f.value, ast.Name) and f.value.id == "torch":
            node.func = ast.copy_location(ast.Name("_recorded_normal", ast.Load()), f)
        return node


def _recorded_normal(mean, std):
    eps = torch.randn(std.shape, generator=REC["gen"])
    REC["eps"] = eps
    return mean + std * eps


def reference_class():
    torch.Tensor.cuda = lambda self, *a, **k: self
    ns = {"torch": torch, "np": np, "nn": nn, "F": F, "_recorded_normal": _recorded_normal,
          "get_expon_lr_func": lambda **kw: (lambda it: 0.0)}
    tree = ast.parse(open(os.path.join(REF, "utils", "general.py")).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("build_rotation", "inverse_sigmoid")]
    assert len(fns) == 2
    mod = ast.fix_missing_locations(_Rewrite().visit(ast.Module(body=fns, type_ignores=[])))
    exec(compile(mod, "<reference utils/general.py>", "exec"), ns)
    tree = ast.parse(open(os.path.join(REF, "models", "gaussian3d.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Gaussian3D"]
    assert len(cls) == 1
    cls[0].bases = []
    cls[0].body = [n for n in cls[0].body if isinstance(n, ast.FunctionDef)]
    mod = ast.fix_missing_locations(_Rewrite().visit(ast.Module(body=cls, type_ignores=[])))
    assert any(isinstance(n, ast.Name) and n.id == "_recorded_normal" for n in ast.walk(mod))
    exec(compile(mod, "<reference models/gaussian3d.py>", "exec"), ns)
    return ns["Gaussian3D"]


class Cfg(dict):
    __getattr__ = dict.get


OPTIM = Cfg(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
            position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)


def levels(g, shape, lo, hi, div):
    """values k / div, k an integer in [lo, hi] without 0"""
    k = torch.randint(lo, hi, shape, generator=g)
    k = torch.where(k >= 0, k + 1, k)
    return k.float() / div


def make_model(G3D, n, rest, seed, planted):
    g = torch.Generator().manual_seed(seed)
    m = G3D(Cfg(sh_degree=3), None, None)
    m.spatial_lr_scale = 1.0
    scaling = 1.2 * torch.randn(n, 3, generator=g) + float(np.log(0.012))
    opacity = 2.0 * torch.randn(n, 1, generator=g)
    for k, (rows, log_scale, logit) in enumerate(planted):
        scaling[rows] = log_scale + 0.2 * torch.randn(len(rows), 3, generator=g)
        opacity[rows] = logit + 0.2 * torch.randn(len(rows), 1, generator=g)
    m._xyz = nn.Parameter(4.0 * torch.rand(n, 3, generator=g) - 2.0)
    m._features_dc = nn.Parameter(levels(g, (n, 1, 3), -16, 16, 32.0))
    m._features_rest = nn.Parameter(levels(g, (n, rest, 3), -16, 16, 32.0))
    m._scaling = nn.Parameter(scaling)
    m._rotation = nn.Parameter(torch.randn(n, 4, generator=g))
    m._opacity = nn.Parameter(opacity)
    m.max_radii2D = torch.zeros(n)
    m.setup_optim(OPTIM)
    loss = sum((levels(g, tuple(p.shape), -8, 8, 16.0) * p).sum() for p in (getattr(m, ATTR[k]) for k in GROUPS))
    loss.backward()
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    return m, g


def snapshot(m, tag, out):
    by = {gr["name"]: gr["params"][0] for gr in m.optimizer.param_groups}
    for name in GROUPS:
        p = by[name]
        assert p is getattr(m, ATTR[name])
        out[f"{tag}_{name}"] = p.detach().numpy().copy()
        st = m.optimizer.state.get(p)
        assert st is not None and float(st["exp_avg"].abs().min()) > 0 or "out" in tag
        out[f"{tag}_{name}_exp_avg"] = st["exp_avg"].numpy().copy()
        out[f"{tag}_{name}_exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
        out[f"{tag}_{name}_step"] = np.asarray(float(st["step"]))
    out[f"{tag}_accum"] = m.xyz_gradient_accum.numpy().copy()
    out[f"{tag}_denom"] = m.denom.numpy().copy()
    out[f"{tag}_max_radii2D"] = m.max_radii2D.numpy().copy()


def away(value, thr, what):
    rel = np.abs(np.asarray(value, np.float64) / thr - 1.0)
    assert rel.min() >= MARGIN, f"{what}: {rel.min():.3e} from its threshold {thr}; pick another seed"
    return float(rel.min())


def densify_case(G3D, tag, rest, seed, max_screen_size, out):
    n, max_grad, min_opacity, extent = 400, 0.0002, 0.005, 1.0
    # planted: low-opacity small Gaussians (pruned originals and, with a high gradient, pruned clones) and low-opacity large ones
    # (split parents whose children are pruned by opacity)
    planted = [(list(range(0, 12)), float(np.log(0.003)), -7.0), (list(range(12, 20)), float(np.log(0.05)), -7.0)]
    m, g = make_model(G3D, n, rest, seed, planted)
    denom = torch.randint(0, 6, (n, 1), generator=g).float()
    grad = max_grad * torch.exp(1.0 * torch.randn(n, 1, generator=g))
    grad[0:6] = max_grad * 3.0            # planted small + low opacity + hot -> pruned clones
    grad[6:12] = max_grad * 0.1           # ... + cold -> pruned originals
    grad[12:20] = max_grad * 3.0          # planted large + low opacity + hot -> split, children pruned
    denom[0:20] = 2.0
    m.xyz_gradient_accum = grad * denom
    m.denom = denom
    m.max_radii2D = torch.randint(0, 60, (n,), generator=g).float()        # some above max_screen_size: it must not matter
    snapshot(m, f"{tag}_in", out)
    # the classes, from the inputs, in float64
    with np.errstate(divide="ignore", invalid="ignore"):
        gq = (m.xyz_gradient_accum / m.denom).numpy().astype(np.float64).reshape(-1)
    gq = np.where(np.isnan(gq), 0.0, gq)
    s = np.exp(m._scaling.detach().numpy().astype(np.float64))
    mx = s.max(1)
    o = 1.0 / (1.0 + np.exp(-m._opacity.detach().numpy().astype(np.float64).reshape(-1)))
    dense, big = OPTIM.percent_dense * extent, 0.1 * extent
    margins = dict(g=away(gq[gq > 0], max_grad, "g"), m_dense=away(mx, dense, "m vs percent_dense extent"),
                   o=away(o, min_opacity, "o"))
    hot = gq >= max_grad
    clone, split = hot & (mx <= dense), hot & (mx > dense)
    use_big = bool(max_screen_size)
    if use_big:
        margins["m_big"] = away(mx, big, "m vs 0.1 extent")
        margins["child_big"] = away(mx / 1.6, big, "child scale vs 0.1 extent")
    gone = (o < min_opacity) | (use_big & (mx > big))
    child_gone = (o < min_opacity) | (use_big & (mx / 1.6 > big))
    classes = {"clones": clone & ~gone, "pruned clones": clone & gone, "split, children survive": split & ~child_gone,
               "split, children pruned": split & child_gone, "pruned originals": ~split & gone, "denom == 0": m.denom.numpy().reshape(-1) == 0}
    for k, v in classes.items():
        assert v.sum() >= 4, f"{tag}: only {v.sum()} {k}; pick another seed"
    assert (m.max_radii2D > 20).sum() >= 4
    m.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)
    snapshot(m, f"{tag}_out", out)
    want_rows = int((~split & ~gone).sum() + (clone & ~gone).sum() + 2 * (split & ~child_gone).sum())
    assert m._xyz.shape[0] == want_rows, (m._xyz.shape[0], want_rows)        # the single-pass count is the reference's
    out[f"{tag}_eps"] = REC["eps"].numpy().copy()
    assert REC["eps"].shape[0] == 2 * int(split.sum())
    out[f"{tag}_settings"] = np.asarray([max_grad, min_opacity, extent, float(max_screen_size or 0), OPTIM.percent_dense], np.float64)
    out[f"{tag}_class_counts"] = np.asarray([int(v.sum()) for v in classes.values()])
    print(tag, {k: int(v.sum()) for k, v in classes.items()}, "rows", n, "->", want_rows, "margins", {k: f"{v:.2e}" for k, v in margins.items()})


def small_cases(G3D, out):
    n = 100
    m, g = make_model(G3D, n, 3, 31, [(list(range(0, 8)), float(np.log(0.003)), -7.0)])
    m.xyz_gradient_accum = torch.rand(n, 1, generator=g)
    m.denom = torch.randint(0, 6, (n, 1), generator=g).float()
    m.max_radii2D = torch.randint(0, 60, (n,), generator=g).float()
    snapshot(m, "prune_in", out)
    o = torch.sigmoid(m._opacity.detach()).numpy().astype(np.float64)
    away(o, 0.005, "opacity_prune o")
    assert 4 <= (o < 0.005).sum() < n
    m.opacity_prune(0.005)
    snapshot(m, "prune_out", out)
    out["prune_min_opacity"] = np.asarray(0.005)

    m, g = make_model(G3D, n, 3, 32, [(list(range(0, 8)), float(np.log(0.003)), -7.0)])
    m.xyz_gradient_accum, m.denom = torch.zeros(n, 1), torch.zeros(n, 1)
    out["reset_in_opacity"] = m._opacity.detach().numpy().copy()
    out["reset_in_scaling"] = m._scaling.detach().numpy().copy()
    o = torch.sigmoid(m._opacity.detach())
    assert 4 <= int((o < 0.01).sum()) and 4 <= int((o > 0.01).sum())
    m.reset_opacity()
    m.reset_min_scale()
    for name in ("opacity", "scaling"):
        p = getattr(m, ATTR[name])
        st = m.optimizer.state[p]
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 1.0
        out[f"reset_out_{name}"] = p.detach().numpy().copy()


def stats_case(G3D, out):
    n = 400
    g = torch.Generator().manual_seed(41)
    m = G3D(Cfg(sh_degree=3), None, None)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.zeros(n, 1), torch.zeros(n, 1), torch.zeros(n)
    for r in range(2):
        class Carrier:
            grad = 1e-3 * torch.randn(n, 3, generator=g)
        radii = torch.randint(1, 40, (n,), generator=g, dtype=torch.int32) * (torch.rand(n, generator=g) < 0.4).int()
        visibility_filter = radii > 0
        # models/gaussian3d.py:431-432
        m.max_radii2D[visibility_filter] = torch.max(m.max_radii2D[visibility_filter], radii[visibility_filter])
        m.add_densification_stats(Carrier, visibility_filter)
        out[f"stats_grad{r}"], out[f"stats_radii{r}"] = Carrier.grad.numpy().copy(), radii.numpy().copy()
        out[f"stats_accum{r}"], out[f"stats_denom{r}"] = m.xyz_gradient_accum.numpy().copy(), m.denom.numpy().copy()
        out[f"stats_max_radii2D{r}"] = m.max_radii2D.numpy().copy()
    both = (out["stats_radii0"] > 0) & (out["stats_radii1"] > 0)
    assert both.sum() >= 4 and ((out["stats_radii0"] <= 0) & (out["stats_radii1"] <= 0)).sum() >= 4


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the file regenerates byte for byte"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    G3D = reference_class()
    REC["gen"] = torch.Generator().manual_seed(7)
    out = {}
    densify_case(G3D, "sh3", 15, 11, 20, out)
    densify_case(G3D, "sh1", 3, 12, None, out)
    small_cases(G3D, out)
    stats_case(G3D, out)
    path = os.path.join(HERE, "density.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    sys.exit(main())
