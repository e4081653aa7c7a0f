"""-m gpu: texgs.density (csrc/density.hip) against its numpy statement (tests/density_ref.py) and against the reference's own results
(tests/golden/density.npz).

Against density_ref: statistics, action bytes, ranks, totals, copied rows and moments are compared for EQUALITY; children's xyz and
scaling within density_ref.TOL_CHILD (2e-6 absolute: numpy's and the device's expf / logf may differ in the last bit).  The test
clouds (density_ref.cloud) keep every compared quantity 1e-4 away from its threshold for the same reason: a decision cannot hang on
the last bit of an expf.  Sizes: around a wave (63..65), around a block (255..257), around what one scan block covers (1023..1025),
and 300 001 -- more than the 256 tiles (262 144 Gaussians) the tile scan takes in one pass."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KW = dict(max_grad=0.0002, min_opacity=0.005, dense_scale=0.01, big_scale=0.1)
ATTRS = ("xyz_gradient_accum", "denom", "max_radii2D")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _state(density, accum, denom, n):
    return density.DensityState(_dev(accum), _dev(denom), torch.zeros(n, device="cuda"))


# ---- statistics ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 100003])
def test_statistics_bit_equal_and_accumulate(lib_built, n):
    from texgs import density
    rng = np.random.RandomState(n)
    st = density.DensityState.zeros(n, "cuda")
    want = (np.zeros((n, 1), np.float32), np.zeros((n, 1), np.float32), np.zeros(n, np.float32))
    for r in range(2):
        grad = (1e-3 * rng.randn(n, 3)).astype(np.float32)
        radii = (rng.randint(1, 40, n) * (rng.rand(n) < 0.4)).astype(np.int32)
        if r == 0:
            radii[0] = 7
        g, rd = _dev(grad), _dev(radii)
        before = tuple(getattr(st, k).data_ptr() for k in ATTRS)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")         # a host synchronisation inside the call raises
        try:
            density.add_densification_stats(st, g, rd)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert before == tuple(getattr(st, k).data_ptr() for k in ATTRS)        # in place
        want = R.stats_np(*want, grad, radii)
        for k, w in zip(ATTRS, want):
            assert np.array_equal(getattr(st, k).cpu().numpy().view(np.uint32), w.view(np.uint32)), (n, r, k)
    assert want[1].max() == 2.0 or n < 10


def test_sync_debug_mode_sees_a_synchronisation():
    """The guard of the test above does something on this build: a readback under it raises."""
    x = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            x.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ---- plan ----
def _plan_both(density, scaling, opacity, accum, denom, **kw):
    n = scaling.shape[0]
    got = density._plan_densify({"scaling": _dev(scaling), "opacity": _dev(opacity)}, _state(density, accum, denom, n), **kw)
    want = R.plan_np(accum, denom, scaling, opacity, **kw)
    return [g.cpu().numpy() for g in got], want


def _assert_plan_equal(got, want, what):
    assert np.array_equal(got[2].astype(np.int64), want[2]), (what, "totals", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "action", int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), (what, "rank")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 300001])
def test_plan_bit_equal(lib_built, n):
    from texgs import density
    params, accum, denom, _ = R.cloud(n, seed=100 + n % 97)
    for use_big in (True, False):
        got, want = _plan_both(density, params["scaling"], params["opacity"], accum, denom, use_big=use_big, **KW)
        _assert_plan_equal(got, want, (n, use_big))
    if n >= 1023:
        assert min(want[2]) > 0             # every count is exercised
    got, want = _plan_both(density, params["scaling"], params["opacity"], accum, denom, densify=False, use_big=False, **KW)
    _assert_plan_equal(got, want, (n, "opacity_prune"))
    assert want[2][1] == want[2][2] == want[2][3] == 0


@pytest.mark.parametrize("case", ["nothing selected", "everything split", "everything pruned", "denom all zero"])
def test_plan_special_cases(lib_built, case):
    from texgs import density
    n = 1500
    params, accum, denom, _ = R.cloud(n, seed=5)
    scaling, opacity = params["scaling"], params["opacity"]
    if case == "nothing selected":
        accum = np.zeros_like(accum)
    elif case == "everything split":
        scaling = np.full((n, 3), math.log(0.05), np.float32)
        opacity = np.full((n, 1), 2.0, np.float32)
        accum, denom = np.full((n, 1), 1.0, np.float32), np.full((n, 1), 2.0, np.float32)
    elif case == "everything pruned":
        opacity = np.full((n, 1), -10.0, np.float32)
    else:                                   # never visible: 0 / 0 is NaN, which counts as 0
        accum, denom = np.zeros_like(accum), np.zeros_like(denom)
    got, want = _plan_both(density, scaling, opacity, accum, denom, use_big=True, **KW)
    _assert_plan_equal(got, want, case)
    k, c, s, ch = (int(v) for v in want[2])
    if case in ("nothing selected", "denom all zero"):
        assert (c, s, ch) == (0, 0, 0) and 0 < k < n
    elif case == "everything split":
        assert (k, c, s, ch) == (0, 0, n, n)
    else:
        assert (k, c, ch) == (0, 0, 0)


# ---- the public functions ----
def _model(params_np, with_state=True, seed=0):
    """Parameters on the GPU under a real torch.optim.Adam; with_state: one step, so that the moments are non-zero"""
    params = {k: torch.nn.Parameter(_dev(params_np[k])) for k in R.GROUPS}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-4, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    if with_state:
        g = torch.Generator(device="cuda").manual_seed(seed)
        for p in params.values():
            p.grad = torch.randn(p.shape, generator=g, device="cuda")
        opt.step()
        opt.zero_grad(set_to_none=True)
    return params, opt


def _snapshot(params, opt):
    pn = {k: p.detach().cpu().numpy().copy() for k, p in params.items()}
    mn = {}
    for k, p in params.items():
        st = opt.state.get(p)
        mn[k] = (st["exp_avg"].cpu().numpy().copy(), st["exp_avg_sq"].cpu().numpy().copy()) if st else None
    return pn, mn


def _check_optimizer(opt, new, m, with_state=True):
    by = {g["name"]: g["params"][0] for g in opt.param_groups}
    assert len(opt.state) == (6 if with_state else 0)
    for k in R.GROUPS:
        assert by[k] is new[k] and isinstance(new[k], torch.nn.Parameter) and new[k].requires_grad and new[k].shape[0] == m
        if with_state:
            st = opt.state[new[k]]
            assert st["exp_avg"].shape == new[k].shape == st["exp_avg_sq"].shape and float(st["step"]) == 1.0


@pytest.mark.parametrize("width_rest, with_state", [(45, True), (9, True), (45, False)])
def test_move_against_the_statement(lib_built, width_rest, with_state):
    from texgs import density
    n = 1500
    params_np, accum, denom, noise_all = R.cloud(n, seed=7 + width_rest, width_rest=width_rest, frac=(0.2, 0.2, 0.1))
    params, opt = _model(params_np, with_state)
    pn, mn = _snapshot(params, opt)         # (the Adam step moved the parameters: the plan is made from what the GPU holds)
    action, rank, totals = R.plan_np(accum, denom, pn["scaling"], pn["opacity"], use_big=True, **KW)
    got_plan = density._plan_densify({"scaling": params["scaling"].detach(), "opacity": params["opacity"].detach()},
                                    _state(density, accum, denom, n), use_big=True, **KW)
    _assert_plan_equal([g.cpu().numpy() for g in got_plan], (action, rank, totals), "move")
    assert min(totals) >= 20 and totals[2] > totals[3]
    noise = noise_all[:2 * totals[2]]
    want, want_m = R.move_np(pn, mn, action, rank, totals, noise)
    st = _state(density, accum, denom, n)
    st.max_radii2D += 100.0                 # above any max_screen_size: must not matter
    new = density.densify_and_prune(params, opt, st, max_grad=KW["max_grad"], min_opacity=KW["min_opacity"], extent=1.0,
                                    max_screen_size=20, percent_dense=0.01, noise=_dev(noise))
    m = int(totals[0] + totals[1] + 2 * totals[3])
    n_copied = int(totals[0] + totals[1])
    _check_optimizer(opt, new, m, with_state)
    for k in R.GROUPS:
        got = new[k].detach().cpu().numpy()
        assert got.shape == want[k].shape
        if k in ("xyz", "scaling"):
            assert np.array_equal(got[:n_copied], want[k][:n_copied]), k
            err = float(np.abs(got[n_copied:].astype(np.float64) - want[k][n_copied:]).max())
            print(f"children {k}: max |error| against the statement {err:.3e}")
            assert err <= R.TOL_CHILD, (k, err)
        else:
            assert np.array_equal(got, want[k]), k
        if with_state:
            for j, mk in enumerate(("exp_avg", "exp_avg_sq")):
                got_m = opt.state[new[k]][mk].cpu().numpy()
                assert np.array_equal(got_m, want_m[k][j]), (k, mk)
                assert not got_m[int(totals[0]):].any() and got_m[:int(totals[0])].any()
    for k in ATTRS:
        t = getattr(st, k)
        assert t.shape[0] == m and t.dim() == (1 if k == "max_radii2D" else 2) and not bool(t.any())


def test_everything_pruned_gives_zero_rows(lib_built):
    from texgs import density
    n = 300
    params_np, accum, denom, _ = R.cloud(n, seed=3, width_rest=9)
    params_np["opacity"] = np.full((n, 1), -10.0, np.float32)
    params, opt = _model(params_np, with_state=False)
    st = _state(density, accum, denom, n)
    new = density.densify_and_prune(params, opt, st, max_grad=0.0002, min_opacity=0.005, extent=1.0, max_screen_size=None,
                                    percent_dense=0.01)
    assert all(new[k].shape == (0,) + tuple(params_np[k].shape[1:]) for k in R.GROUPS) and st.denom.shape == (0, 1)
    again = density.opacity_prune(new, opt, st, 0.005)            # and a call on the empty model is no error either
    assert again["xyz"].shape == (0, 3)


def test_generator_draws_the_noise(lib_built):
    """noise=None: the samples come from torch.randn(generator=...) on the device -- the same seed gives the same children, and
    they are the children of that noise passed explicitly."""
    from texgs import density
    n = 700
    params_np, accum, denom, _ = R.cloud(n, seed=9, width_rest=9, frac=(0.2, 0.2, 0.1))
    kw = dict(max_grad=0.0002, min_opacity=0.005, extent=1.0, max_screen_size=20, percent_dense=0.01)
    outs = []
    for mode in ("gen", "gen", "explicit"):
        params, opt = _model(params_np, with_state=False)
        gen = torch.Generator(device="cuda").manual_seed(123)
        if mode == "explicit":
            ns = int(R.plan_np(accum, denom, params_np["scaling"], params_np["opacity"], use_big=True, **KW)[2][2])
            extra = dict(noise=torch.randn((2 * ns, 3), generator=gen, dtype=torch.float32, device="cuda"))
        else:
            extra = dict(generator=gen)
        outs.append(density.densify_and_prune(params, opt, _state(density, accum, denom, n), **kw, **extra)["xyz"].detach())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    with pytest.raises(ValueError, match="noise must be"):
        params, opt = _model(params_np, with_state=False)
        density.densify_and_prune(params, opt, _state(density, accum, denom, n), noise=torch.zeros(4, 3, device="cuda"), **kw)


# ---- the reference's own results, end to end through the public functions ----
def _golden_model(tag):
    G = R.golden()
    params_np, moments, accum, denom = R.golden_case(tag)
    params, opt = _model(params_np, with_state=False)
    for k, p in params.items():
        opt.state[p] = {"step": torch.tensor(float(G[f"{tag}_in_{k}_step"])), "exp_avg": _dev(moments[k][0]), "exp_avg_sq": _dev(moments[k][1])}
    from texgs import density
    st = density.DensityState(_dev(accum), _dev(denom), _dev(G[f"{tag}_in_max_radii2D"]))
    return params, opt, st


def _step_and_check_rows(opt, new, m):
    for p in new.values():
        p.grad = torch.ones_like(p)
    opt.step()
    for p in new.values():
        st = opt.state[p]
        assert st["exp_avg"].shape[0] == m and st["exp_avg_sq"].shape[0] == m and float(st["step"]) == 2.0 and p.shape[0] == m


@pytest.mark.parametrize("tag", ["sh3", "sh1"])
def test_golden_densify_and_prune(lib_built, tag):
    from texgs import density
    G = R.golden()
    params, opt, st = _golden_model(tag)
    max_grad, min_opacity, extent, max_screen_size, percent_dense = (float(v) for v in G[f"{tag}_settings"])
    new = density.densify_and_prune(params, opt, st, max_grad=max_grad, min_opacity=min_opacity, extent=extent,
                                    max_screen_size=max_screen_size or None, percent_dense=percent_dense, noise=_dev(G[f"{tag}_eps"]))
    m = G[f"{tag}_out_xyz"].shape[0]
    _check_optimizer(opt, new, m)
    pn, mn = _snapshot(new, opt)
    counts = G[f"{tag}_class_counts"]
    n_children = 2 * int(counts[2])
    R.check_against_golden(tag, pn, mn, m - n_children, "GPU")
    for k in ATTRS:
        assert getattr(st, k).shape[0] == m and not bool(getattr(st, k).any())
    _step_and_check_rows(opt, new, m)


def test_golden_opacity_prune(lib_built):
    from texgs import density
    G = R.golden()
    params, opt, st = _golden_model("prune")
    new = density.opacity_prune(params, opt, st, float(G["prune_min_opacity"]))
    m = G["prune_out_xyz"].shape[0]
    _check_optimizer(opt, new, m)
    pn, mn = _snapshot(new, opt)
    R.check_against_golden("prune", pn, mn, m, "GPU")
    for k, name in zip(ATTRS, ("accum", "denom", "max_radii2D")):
        assert np.array_equal(getattr(st, k).cpu().numpy(), G[f"prune_out_{name}"]), k
    _step_and_check_rows(opt, new, m)


def test_golden_resets(lib_built):
    from texgs import density
    G = R.golden()
    n = G["reset_in_opacity"].shape[0]
    params_np, _, _, _ = R.cloud(n, seed=1, width_rest=9)
    params_np["opacity"], params_np["scaling"] = G["reset_in_opacity"], G["reset_in_scaling"]
    params, opt = _model(params_np, with_state=False)
    for p in params.values():
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # element-wise torch on the device: nothing is read back
    try:
        new_o = density.reset_opacity(params, opt)
        params["opacity"] = new_o
        new_s = density.reset_min_scale(params, opt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    err = float(np.abs(new_o.detach().cpu().numpy().astype(np.float64) - G["reset_out_opacity"]).max())
    print(f"reset_opacity: max |error| {err:.3e} (bound 2e-6)")
    assert err <= 2e-6
    assert np.array_equal(new_s.detach().cpu().numpy(), G["reset_out_scaling"])
    by = {g["name"]: g["params"][0] for g in opt.param_groups}
    assert by["opacity"] is new_o and by["scaling"] is new_s and len(opt.state) == 6
    for p in (new_o, new_s):
        st = opt.state[p]
        assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()) and float(st["step"]) == 1.0
    assert bool(opt.state[by["xyz"]]["exp_avg"].all())          # the other groups are untouched


def test_golden_statistics(lib_built):
    from texgs import density
    G = R.golden()
    n = G["stats_radii0"].shape[0]
    st = density.DensityState.zeros(n, "cuda")
    for r in range(2):
        density.add_densification_stats(st, _dev(G[f"stats_grad{r}"]), _dev(G[f"stats_radii{r}"]))
        want = G[f"stats_accum{r}"].astype(np.float64)
        rel = float((np.abs(st.xyz_gradient_accum.cpu().numpy().astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)).max())
        print(f"statistics round {r}: max relative error of the accumulated norms {rel:.3e} (bound {R.TOL_NORM:.0e})")
        assert rel <= R.TOL_NORM
        assert np.array_equal(st.denom.cpu().numpy(), G[f"stats_denom{r}"])
        assert np.array_equal(st.max_radii2D.cpu().numpy(), G[f"stats_max_radii2D{r}"])


# ---- the rasterizer's caches cannot serve an entry from before the call ----
def test_rasterizer_caches_after_densify(lib_built):
    """N = 2000 at 64 x 64 through diff_gauss: render + backward, statistics, densify_and_prune, render + backward again.  The
    prefetch key holds every tensor's storage, version and shape and a pending forward keeps its tensors alive; the shared-geometry
    entry is compared by N and by the new forward's own fingerprint -- so the second image must be the image of fresh clones."""
    import diff_gauss as dg
    import helpers as Hh
    from texgs import density, synth
    import torch.nn.functional as F
    n = 2000
    scene = synth.make_scene(n, 4, seed=17, scale_mean=0.05)
    cam = synth.fibonacci_cameras(4, 64, 64)[1]
    dev = torch.device("cuda:0")
    st_gpu = Hh.settings_for(cam, 3, torch.tensor([0.1, 0.0, 0.2]), device=dev, cls=dg.GaussianRasterizationSettings)
    g = torch.Generator().manual_seed(2)
    params_np = {"xyz": scene.means3D.numpy(), "f_dc": torch.randn(n, 1, 3, generator=g).numpy(), "f_rest": scene.shs.numpy(),
                 "opacity": torch.logit(scene.opacities).numpy(), "scaling": torch.log(scene.scales).numpy(),
                 "rotation": scene.rotations.numpy()}
    params, opt = _model(params_np, with_state=True)

    def render(p):
        m2 = torch.zeros(p["xyz"].shape[0], 3, device=dev, requires_grad=True)
        out = dg.GaussianRasterizer(st_gpu)(means3D=p["xyz"], means2D=m2, opacities=torch.sigmoid(p["opacity"]),
                                            shs=torch.cat((p["f_dc"], p["f_rest"]), dim=1), scales=torch.exp(p["scaling"]),
                                            rotations=F.normalize(p["rotation"]), cov3Ds_precomp=None, extra_attrs=None)
        (out[0].square().sum() + out[3].sum()).backward()
        return out[0].detach().clone(), out[4], m2.grad

    image0, radii0, vgrad = render(params)
    assert radii0.shape == (n,) and radii0.dtype == torch.int32 and int((radii0 > 0).sum()) > n // 4
    state = density.DensityState.zeros(n, "cuda")
    density.add_densification_stats(state, vgrad, radii0)
    vis = radii0 > 0
    assert bool((state.denom[:, 0] == vis.float()).all()) and bool((state.max_radii2D == radii0.clamp_min(0).float()).all())
    norms = state.xyz_gradient_accum[vis, 0]
    assert float(norms.max()) > 0
    max_grad = float(norms.median())
    new = density.densify_and_prune(params, opt, state, max_grad=max_grad, min_opacity=0.005, extent=5.0, max_screen_size=20,
                                    percent_dense=0.01, generator=torch.Generator(device="cuda").manual_seed(4))
    m = new["xyz"].shape[0]
    assert m > n + n // 20                      # about half of the visible ones were cloned or split
    image1, radii1, vgrad1 = render(new)
    assert radii1.shape == (m,) and vgrad1.shape == (m, 3) and state.N == m
    fresh = {k: v.detach().clone().requires_grad_(True) for k, v in new.items()}
    image2, radii2, _ = render(fresh)
    assert torch.equal(image1, image2) and torch.equal(radii1, radii2)
    assert not torch.equal(image1, image0)
    opt.step()                                  # the optimizer steps the new parameters with their new moments
    assert all(opt.state[p]["exp_avg"].shape[0] == m for p in new.values())
