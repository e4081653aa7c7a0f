"""-m gpu: texgs.optim (csrc/optim.hip) against its numpy statement (tests/adam_ref.py), bit for bit, and against torch's own Adam on
the device in scaled units.

Bit identity: p, exp_avg and exp_avg_sq are compared as int32 patterns (NaNs by position) after each of 3 steps, with non-zero moments
from the first step on.  Sizes lie around the kernel's chunk C (one 16-byte access per lane of a 256-thread workgroup): 1, 3, 4, 5
(below, at and above one 16-byte group), 255, 1021, C-1, C, C+1, 2C+3, and 2^21+5 -- 2049 chunks, one more than the grid cap of 2048
workgroups, so the grid-stride loop runs.  Record counts 1, 32, 33, 65 cross the 32-record table of one launch.

torch on the device: the same inputs and metric as tests/test_optim_host.py (adam_ref.parity_inputs / scaled_units, one-step
differences).  m' and v' <= 4 units; the p' bound is twice what profiles/optim_parity.json records (scripts/optim_parity.py measured it
with `measure_parity` below), and may not exceed 16."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-15
# profiles/optim_parity.json: the largest p' difference from torch's Adam on the device (either yardstick), in units of 2^-24 of
# max(|p|, |p' - p|), was PARITY_P_MEASURED; the bound is twice that, for another input seed, and at most 16 (seven roundings a side)
PARITY_P_MEASURED = 5.73
PARITY_P_BOUND = min(2.0 * PARITY_P_MEASURED, 16.0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Spec:
    """One tensor of a call: start values, per-step gradients, hyper-parameters, and the element offsets at which p, g, m, v sit in
    their own flat device buffers (16-byte aligned at offset 0)."""

    def __init__(self, n, seed=0, step0=0, lr=LR, betas=BETAS, eps=EPS, offsets=(0, 0, 0, 0), steps=3):
        rng = np.random.RandomState(1000 + seed)
        self.n, self.step0, self.lr, self.betas, self.eps, self.offsets = n, step0, lr, betas, eps, offsets
        self.p = rng.randn(n).astype(np.float32)
        self.m = (1e-2 * rng.randn(n)).astype(np.float32)
        self.v = (1e-4 * rng.rand(n)).astype(np.float32)
        self.grads = [(10.0 ** rng.uniform(-6, 0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(steps)]


def _slice(values, off):
    buf = torch.zeros(values.size + off + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + values.size]
    t.copy_(torch.from_numpy(values))
    return t


def _build(specs, optim):
    """-> (FusedAdam with one group per spec and the state preset to (step0, m, v), the parameters)"""
    params = [torch.nn.Parameter(_slice(s.p, s.offsets[0])) for s in specs]
    opt = optim.FusedAdam([{"params": [p], "lr": s.lr, "betas": s.betas, "eps": s.eps} for p, s in zip(params, specs)], lr=0.0)
    for p, s in zip(params, specs):
        p.grad = _slice(np.zeros(s.n, np.float32), s.offsets[1])
        opt.state[p] = {"step": torch.tensor(float(s.step0)), "exp_avg": _slice(s.m, s.offsets[2]), "exp_avg_sq": _slice(s.v, s.offsets[3])}
        for t, off in zip((p, p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]), s.offsets):
            assert s.n == 0 or t.data_ptr() % 16 == 4 * off
    return opt, params


def _run_and_compare(specs, optim, zero_grads=False, steps=3):
    """Steps the tensors on the device and in the statement, comparing the bits of p, m, v after every step.  -> the final (p, m, v)
    per spec as numpy, and the optimizer"""
    opt, params = _build(specs, optim)
    want = [(s.p, s.m, s.v, s.step0) for s in specs]
    for k in range(steps):
        for p, s in zip(params, specs):
            p.grad.copy_(torch.from_numpy(s.grads[k]))
        ptrs = [(p.data_ptr(), p.grad.data_ptr()) for p in params]
        opt.step(zero_grads=zero_grads)
        assert ptrs == [(p.data_ptr(), p.grad.data_ptr()) for p in params]          # in place
        want = R.step_np([(w[0], s.grads[k], w[1], w[2], w[3], s.lr, s.betas, s.eps) for w, s in zip(want, specs)])
        for i, (p, s, w) in enumerate(zip(params, specs, want)):
            st = opt.state[p]
            got = (p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
            for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), got, w[:3]):
                assert R.same_bits(a, b), (f"tensor {i} (n={s.n}, offsets={s.offsets}) step {k}: {name} differs in "
                                           f"{int((a.view(np.int32) != b.view(np.int32)).sum())} of {s.n} elements")
            assert float(st["step"]) == w[3] and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
            g = p.grad.cpu().numpy()
            if zero_grads:
                assert not g.view(np.int32).any(), (i, k, "gradient not +0.0 everywhere")
            else:
                assert R.same_bits(g, s.grads[k]), (i, k, "gradient changed")
    return [(p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy()) for p in params], opt


def _sizes(optim):
    c = optim.CHUNK
    return [1, 3, 4, 5, 255, 1021, c - 1, c, c + 1, 2 * c + 3, 2 ** 21 + 5]


@pytest.mark.parametrize("k", range(11))
def test_sizes_bit_equal(lib_built, k):
    from texgs import optim
    n = _sizes(optim)[k]
    assert optim.CHUNK == 1024 and (2 ** 21 + 5 + optim.CHUNK - 1) // optim.CHUNK == 2049           # one chunk past the grid cap
    opt, params = _build([Spec(n, seed=k)], optim)
    params[0].grad.fill_(0.5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")             # a host synchronisation inside step() raises: it reads nothing back
    try:
        opt.step()
        opt.step(zero_grads=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _run_and_compare([Spec(n, seed=k)], optim)


def test_zero_numel_tensor_in_the_middle(lib_built):
    from texgs import optim
    _run_and_compare([Spec(5, seed=1), Spec(0, seed=2), Spec(1021, seed=3)], optim)


@pytest.mark.parametrize("count", [1, 32, 33, 65])
def test_record_counts_cross_the_launch_table(lib_built, count):
    from texgs import optim
    c = optim.CHUNK
    sizes = [1, 3, 4, 5, 255, 1021, c - 1, c, c + 1, 2 * c + 3, 0, 7]
    specs = [Spec(sizes[i % len(sizes)], seed=50 + i, step0=i % 5, lr=LR * (1 + i % 3), offsets=(0, i % 4, 0, 0)) for i in range(count)]
    _run_and_compare(specs, optim, steps=2)


# p, g, m, v at element offsets 0..3 of their buffers: the four rotations leave all four mutually misaligned; then one pointer alone
# off the boundary (a GradBucket slice under aligned parameters), and all four off it by the same amount
@pytest.mark.parametrize("offsets", [(0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (0, 1, 0, 0), (0, 0, 0, 3), (2, 2, 2, 2)])
def test_alignment(lib_built, offsets):
    from texgs import optim
    c = optim.CHUNK
    _run_and_compare([Spec(n, seed=70 + i, offsets=offsets) for i, n in enumerate([2 * c + 3, 5, c])], optim)


def test_grad_bucket_slices(lib_built):
    """A real GradBucket: the gradients are slices of one flat buffer at element offsets 0, 7 and 28; with zero_grads the whole
    buffer is zero afterwards."""
    from texgs import multiview, optim
    rng = np.random.RandomState(5)
    shapes = [(7, 1), (7, 3), (7, 4)]
    for zero in (False, True):
        params = [torch.nn.Parameter(_dev(rng.randn(*s).astype(np.float32))) for s in shapes]
        bucket = multiview.GradBucket(params)
        assert [p.grad.data_ptr() - bucket.flat.data_ptr() for p in params] == [0, 28, 112]
        opt = optim.FusedAdam(params, lr=LR, eps=EPS)
        want = [(p.detach().cpu().numpy().reshape(-1), np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32), 0) for p in params]
        for k in range(3):
            grads = [rng.randn(p.numel()).astype(np.float32) for p in params]
            bucket.flat.copy_(torch.from_numpy(np.concatenate(grads)))
            opt.step(zero_grads=zero)
            want = R.step_np([(w[0], g, w[1], w[2], w[3], LR, BETAS, EPS) for w, g in zip(want, grads)])
            for p, w in zip(params, want):
                st = opt.state[p]
                assert st["exp_avg"].shape == p.shape
                assert R.same_bits(p.detach().cpu().numpy().reshape(-1), w[0])
                assert R.same_bits(st["exp_avg"].cpu().numpy().reshape(-1), w[1]) and R.same_bits(st["exp_avg_sq"].cpu().numpy().reshape(-1), w[2])
                assert p.grad.data_ptr() - bucket.flat.data_ptr() in (0, 28, 112)           # still the bucket's slices
            flat = bucket.flat.cpu().numpy()
            assert (not flat.view(np.int32).any()) if zero else R.same_bits(flat, np.concatenate(grads))


def _value_case(case, n, seed):
    rng = np.random.RandomState(seed)
    s = Spec(n, seed=seed)
    sign = rng.choice([-1.0, 1.0], n)
    if case == "g zero, moments not":
        s.grads = [np.zeros(n, np.float32) for _ in range(3)]
    elif case == "all zero":
        s.grads = [np.zeros(n, np.float32) for _ in range(3)]
        s.m, s.v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    elif case == "tiny g":             # g*g is subnormal or underflows; the moments start at zero so that nothing hides it
        s.grads = [(10.0 ** rng.uniform(-23, -19, n) * sign).astype(np.float32) for _ in range(3)]
        s.m, s.v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    elif case == "tiny g, small moments":
        s.grads = [(10.0 ** rng.uniform(-23, -19, n) * sign).astype(np.float32) for _ in range(3)]
        s.m, s.v = (1e-21 * rng.randn(n)).astype(np.float32), (10.0 ** rng.uniform(-44, -38, n)).astype(np.float32)
    elif case == "huge g":             # g*g is past the largest f32; in the contract's order, (w2*g)*g = 1e37, it is not formed
        s.grads = [(1e20 * sign).astype(np.float32) for _ in range(3)]
    elif case == "overflowing g":      # (w2*g)*g overflows too: v' = inf, den = inf, the update is m'/inf = 0
        s.grads = [(1e30 * sign).astype(np.float32) for _ in range(3)]
    else:                               # single non-finite gradients in the first step
        assert case == "inf and nan"
        for j, bad in ((2, np.inf), (n // 2, -np.inf), (n - 2, np.nan), (min(n - 1, 1029), np.inf)):
            s.grads[0][j] = bad
    return s


@pytest.mark.parametrize("case", ["g zero, moments not", "all zero", "tiny g", "tiny g, small moments", "huge g", "overflowing g", "inf and nan"])
def test_values(lib_built, case):
    from texgs import optim
    n = 2 * optim.CHUNK + 3
    specs = [_value_case(case, n, 90), _value_case(case, n, 91)]
    specs[1].offsets = (0, 1, 0, 0)            # the same values through the 4-byte path
    out, _ = _run_and_compare(specs, optim)
    for s, (p, m, v) in zip(specs, out):
        if case == "all zero":
            assert R.same_bits(p, s.p) and not m.view(np.int32).any() and not v.view(np.int32).any()     # p bit-unchanged
        if case == "g zero, moments not":
            assert m.any() and v.any() and not R.same_bits(p, s.p)
        if case == "tiny g":
            sub = np.abs(v[v != 0]) < R.TINY
            assert sub.any() and (v == 0).any(), "no subnormal and no underflowed second moment: the case tests nothing"
        if case == "huge g":
            assert np.isfinite(v).all() and v.min() > 1e36 and np.isfinite(m).all() and np.isfinite(p).all()
        if case == "overflowing g":
            assert np.isinf(v).all() and np.isfinite(m).all() and R.same_bits(p, s.p)
        if case == "inf and nan":
            bad = np.zeros(n, bool)
            bad[[2, n // 2, n - 2, min(n - 1, 1029)]] = True
            assert not np.isfinite(p[bad]).any() and np.isfinite(p[~bad]).all() and np.isfinite(m[~bad]).all() and np.isfinite(v[~bad]).all()


@pytest.mark.parametrize("betas, eps", [((0.3, 0.999), 1e-15), ((0.3, 0.99), 1e-8), ((0.9, 0.999), 1e-8), ((0.5, 0.9), 1e-15)])
def test_other_lerp_branch_and_eps(lib_built, betas, eps):
    """beta1 = 0.3 gives w1 = 0.7 >= 0.5: torch's lerp interpolates from the other end"""
    from texgs import optim
    assert (R.scalars(1, LR, betas, eps)[0] >= 0.5) == (betas[0] <= 0.5)
    n = optim.CHUNK + 5
    _run_and_compare([Spec(n, seed=3, betas=betas, eps=eps), Spec(n, seed=4, betas=betas, eps=eps, offsets=(1, 0, 0, 0))], optim)


def test_per_tensor_step_values_differ_within_one_call(lib_built):
    from texgs import optim
    steps0 = [0, 1, 10, 1000, 39999]
    _, opt = _run_and_compare([Spec(300 + i, seed=20 + i, step0=s0) for i, s0 in enumerate(steps0)], optim)
    assert [float(st["step"]) for st in opt.state.values()] == [s0 + 3.0 for s0 in steps0]


def test_zero_grads_changes_nothing_else(lib_built):
    from texgs import optim
    c = optim.CHUNK
    mk = lambda: [Spec(n, seed=30 + i, offsets=off) for i, (n, off) in enumerate([(2 * c + 3, (0, 0, 0, 0)), (c + 1, (0, 3, 0, 0)), (0, (0, 0, 0, 0)),
                                                                                    (5, (0, 0, 0, 0)), (255, (1, 2, 3, 0))])]
    plain, _ = _run_and_compare(mk(), optim, zero_grads=False)
    zeroed, _ = _run_and_compare(mk(), optim, zero_grads=True)          # (asserts that every g is +0.0 after each step)
    for a, b in zip(plain, zeroed):
        assert all(R.same_bits(x, y) for x, y in zip(a, b))


def test_fused_step_equals_three_steps(lib_built):
    """Three optimizers -- the shapes of the reference's optimizer / optimizer_uv / optimizer_tex -- through one fused_step call
    end bit-equal to three step() calls, and every counter has advanced by one."""
    from texgs import optim
    rng = np.random.RandomState(8)
    shapes = [[(40, 3), (40, 1), (40, 3), (40, 4), (40, 15, 3)], [(4096,), (1, 128), (2049,)], [(6, 4, 4, 3)]]
    lrs = [1.6e-4, 2e-5, 2.5e-3]
    values = [[rng.randn(*s).astype(np.float32) for s in group] for group in shapes]
    grads = [[[rng.randn(*s).astype(np.float32) for s in group] for group in shapes] for _ in range(2)]
    results = []
    for fused in (False, True):
        opts = []
        for group, lr in zip(values, lrs):
            ps = [torch.nn.Parameter(_dev(x)) for x in group]
            opts.append(optim.FusedAdam([{"params": [p], "name": str(i)} for i, p in enumerate(ps)], lr=lr, eps=EPS))
        for k in range(2):
            for o, gg in zip(opts, grads[k]):
                for group, g in zip(o.param_groups, gg):
                    group["params"][0].grad = _dev(g)
            if k == 1:
                opts[1].param_groups[0]["lr"] = 7e-6            # a scheduler's edit is read at call time
            if fused:
                assert optim.fused_step(opts, zero_grads=True) is None
            else:
                for o in opts:
                    o.step(zero_grads=True)
            for o in opts:
                assert all(float(st["step"]) == k + 1.0 for st in o.state.values()) and len(o.state) == len(o.param_groups)
                assert all(not bool(group["params"][0].grad.any()) for group in o.param_groups)
        results.append([[(g["params"][0].detach().cpu().numpy(), o.state[g["params"][0]]["exp_avg"].cpu().numpy(),
                          o.state[g["params"][0]]["exp_avg_sq"].cpu().numpy()) for g in o.param_groups] for o in opts])
    for a, b in zip(results[0], results[1]):
        for x, y in zip(a, b):
            assert all(R.same_bits(u, w) for u, w in zip(x, y))
    assert not R.same_bits(results[0][0][0][0], values[0][0])


def test_state_made_by_fused_adam_steps_under_torch(lib_built):
    """The state FusedAdam creates is what torch's single-tensor path creates: a plain Adam loads it and steps on"""
    from texgs import optim
    p = torch.nn.Parameter(torch.randn(300, 3, device="cuda"))
    o = optim.FusedAdam([p], lr=LR, eps=EPS)
    p.grad = torch.randn_like(p)
    o.step()
    st = o.state[p]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].shape == () and float(st["step"]) == 1.0
    assert st["exp_avg"].shape == p.shape and st["exp_avg"].device == p.device and bool(st["exp_avg"].any())
    q = torch.nn.Parameter(p.detach().clone())
    plain = torch.optim.Adam([q], lr=LR, eps=EPS)
    plain.load_state_dict(o.state_dict())
    q.grad = torch.randn_like(q)
    plain.step()
    assert float(plain.state[q]["step"]) == 2.0
    o.load_state_dict(plain.state_dict())
    p.grad = torch.randn_like(p)
    o.step()
    assert float(o.state[p]["step"]) == 3.0


# ---- torch's own Adam on the device ----
YARDSTICKS = {"torch default": {}, "torch foreach=False": {"foreach": False}}


def measure_parity(n=65536, steps=8, seed=1):
    """One-step differences in units of 2^-24 of a scale (adam_ref.scaled_units), worst over `steps` steps, the state taken over
    from the yardstick after every step: FusedAdam against torch.optim.Adam on the device (its defaults, and foreach=False), and
    torch's CPU Adam against the same -- the reference's own spread.  -> {yardstick: {"ours": [p, m, v], "torch_cpu": [p, m, v]}}"""
    from texgs import optim
    out = {}
    for name, kw in YARDSTICKS.items():
        p_np, grad = R.parity_inputs(n, seed=seed)
        pt = torch.nn.Parameter(_dev(p_np))
        ot = torch.optim.Adam([pt], lr=LR, betas=BETAS, eps=EPS, **kw)
        po = torch.nn.Parameter(_dev(p_np))
        oo = optim.FusedAdam([po], lr=LR, betas=BETAS, eps=EPS)
        pc = torch.nn.Parameter(torch.from_numpy(p_np.copy()))
        oc = torch.optim.Adam([pc], lr=LR, betas=BETAS, eps=EPS, **kw)
        worst = {"ours": np.zeros(3), "torch_cpu": np.zeros(3)}
        for k in range(steps):
            g = grad(k)
            st = ot.state.get(pt)
            p0 = pt.detach().cpu().numpy().copy()
            m0 = st["exp_avg"].cpu().numpy().copy() if st else np.zeros(n, np.float32)
            v0 = st["exp_avg_sq"].cpu().numpy().copy() if st else np.zeros(n, np.float32)
            with torch.no_grad():
                po.copy_(_dev(p0))
                pc.copy_(torch.from_numpy(p0))
            oo.state[po] = {"step": torch.tensor(float(k)), "exp_avg": _dev(m0), "exp_avg_sq": _dev(v0)}
            oc.state[pc] = {"step": torch.tensor(float(k)), "exp_avg": torch.from_numpy(m0.copy()), "exp_avg_sq": torch.from_numpy(v0.copy())}
            for p, o in ((pt, ot), (po, oo), (pc, oc)):
                p.grad = torch.from_numpy(g.copy()).to(p.device)
                o.step()
            res = lambda p, o: (p.detach().cpu().numpy(), o.state[p]["exp_avg"].cpu().numpy(), o.state[p]["exp_avg_sq"].cpu().numpy())
            want = res(pt, ot)
            assert float(ot.state[pt]["step"]) == float(oo.state[po]["step"]) == float(oc.state[pc]["step"]) == k + 1.0
            worst["ours"] = np.maximum(worst["ours"], R.scaled_units(p0, g, m0, v0, res(po, oo), want))
            worst["torch_cpu"] = np.maximum(worst["torch_cpu"], R.scaled_units(p0, g, m0, v0, res(pc, oc), want))
        out[name] = {k: [float(x) for x in v] for k, v in worst.items()}
    return out


def test_parity_with_torch_adam_on_the_device(lib_built):
    got = measure_parity()
    for name, r in got.items():
        print(f"{name}: FusedAdam p' {r['ours'][0]:.2f}  m' {r['ours'][1]:.2f}  v' {r['ours'][2]:.2f} units;  torch CPU against torch GPU "
              f"p' {r['torch_cpu'][0]:.2f}  m' {r['torch_cpu'][1]:.2f}  v' {r['torch_cpu'][2]:.2f} units  (p' bound {PARITY_P_BOUND:.1f})")
    assert PARITY_P_BOUND <= 16.0
    for name, r in got.items():
        assert r["ours"][1] <= 4.0 and r["ours"][2] <= 4.0, (name, r)
        assert r["ours"][0] <= PARITY_P_BOUND, (name, r)


# ---- composition with density control ----
def test_moments_through_densify_and_prune(lib_built):
    """Step, densify_and_prune at N = 64, step again: the moments of the surviving rows (and of the new ones, which start at zero
    under the group's old step count) follow the statement bit for bit."""
    import density_ref as D
    from texgs import density, optim
    n = 64
    kw = dict(max_grad=0.0002, min_opacity=0.005, dense_scale=0.01, big_scale=0.1)
    params_np, accum, denom, noise_all = D.cloud(n, seed=11, width_rest=9, frac=(0.2, 0.2, 0.1))
    params = {k: torch.nn.Parameter(_dev(params_np[k])) for k in D.GROUPS}
    lrs = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=1.25e-4, opacity=0.05, scaling=5e-3, rotation=1e-3)
    opt = optim.FusedAdam([{"params": [p], "lr": lrs[k], "name": k} for k, p in params.items()], lr=0.0, eps=EPS)
    rng = np.random.RandomState(12)
    flat = lambda t: t.detach().cpu().numpy().reshape(-1)

    g1 = {k: (1e-3 * rng.randn(*params_np[k].shape)).astype(np.float32) for k in D.GROUPS}
    for k, p in params.items():
        p.grad = _dev(g1[k])
    opt.step()
    want = {k: R.step_np([(params_np[k].reshape(-1), g1[k].reshape(-1), np.zeros(params_np[k].size, np.float32),
                           np.zeros(params_np[k].size, np.float32), 0, lrs[k], BETAS, EPS)])[0] for k in D.GROUPS}
    for k, p in params.items():
        assert R.same_bits(flat(p), want[k][0]) and R.same_bits(flat(opt.state[p]["exp_avg"]), want[k][1])

    mk_state = lambda: density.DensityState(_dev(accum), _dev(denom), torch.zeros(n, device="cuda"))
    action = density._plan_densify({"scaling": params["scaling"].detach(), "opacity": params["opacity"].detach()}, mk_state(),
                                   use_big=True, **kw)[0].cpu().numpy()
    kept = np.flatnonzero(action & D.KEEP)
    new = density.densify_and_prune(params, opt, mk_state(), max_grad=kw["max_grad"], min_opacity=kw["min_opacity"], extent=1.0,
                                    max_screen_size=20, percent_dense=0.01, generator=torch.Generator(device="cuda").manual_seed(3))
    m = new["xyz"].shape[0]
    assert 0 < kept.size < n and m > kept.size and m != n           # rows went and rows came
    assert isinstance(opt, torch.optim.Adam) and all(float(opt.state[p]["step"]) == 1.0 for p in new.values())

    g2, expect = {}, {}
    for k, p in new.items():
        width = int(np.prod(params_np[k].shape[1:]))
        rows = lambda a: np.concatenate([a.reshape(n, width)[kept], np.zeros((m - kept.size, width), np.float32)]).reshape(-1)
        m_in, v_in = rows(want[k][1]), rows(want[k][2])
        st = opt.state[p]
        assert R.same_bits(flat(st["exp_avg"]), m_in) and R.same_bits(flat(st["exp_avg_sq"]), v_in)      # what the move left
        g2[k] = (1e-3 * rng.randn(*p.shape)).astype(np.float32)
        expect[k] = R.step_np([(flat(p), g2[k].reshape(-1), m_in, v_in, 1, lrs[k], BETAS, EPS)])[0]
        p.grad = _dev(g2[k])
    optim.fused_step([opt], zero_grads=True)
    for k, p in new.items():
        st = opt.state[p]
        assert float(st["step"]) == 2.0 and st["exp_avg"].shape == p.shape
        assert R.same_bits(flat(st["exp_avg"]), expect[k][1]) and R.same_bits(flat(st["exp_avg_sq"]), expect[k][2]), k
        assert R.same_bits(flat(p), expect[k][0]), k
        assert bool(st["exp_avg"].reshape(m, -1)[:kept.size].any()) and not bool(p.grad.any())
