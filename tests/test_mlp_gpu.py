"""-m gpu: the fused MLP (csrc/mlp.hip through texgs.mlp) and the tinycudann / pytorch3d drop-ins on the MI355X.

Every compared tensor t:   max|hip - f64| <= 4 x max( max|cpu_f32 - f64|, 2^-23 max|f64| )      (mlp_ref.tolerance)
f64 is tests/mlp_ref.py's float64 statement, cpu_f32 the same chain in float32 on the CPU: the 4x over another fp32 evaluation's own error
is the margin tests/test_preprocess_gpu.py uses; the floor keeps an exactly representable case from demanding zero.  Inputs come from
mlp_ref.kink_free_inputs, so no ReLU mask can differ between the evaluations and no row is excluded anywhere.  Edge sizes are derived
from the tile constants texgs.mlp exports.  scripts/mlp_parity.py writes the measured ratios to profiles/mlp_parity.json."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch
from torch import nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SPECS = [(3, 128, 1), (32, 128, 1), (128, 3, 2), (128, 128, 2), (16, 16, 1), (1, 1, 2), (17, 33, 2)]
_id = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)
NETCFG = lambda depth: {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128, "n_hidden_layers": depth}


def _sizes(tile):
    return [1, tile - 1, tile, tile + 1, 2 * tile + 1]


@functools.lru_cache(maxsize=None)
def _case(spec, N):
    """Inputs and both CPU evaluations of a case, computed once and shared (read-only)"""
    params, x = R.kink_free_inputs(spec, N, seed=11 + N)
    dy = np.random.default_rng(5 + N).standard_normal((N, spec[1])).astype(np.float32)
    dx64, dp64 = R.backward(params, x, dy, spec)
    dx32, dp32 = R.backward(params, x, dy, spec, fp32=True)
    out = dict(params=params, x=x, dy=dy, y64=R.forward(params, x, spec), y32=R.forward(params, x, spec, fp32=True), dx64=dx64, dp64=dp64,
               dx32=dx32, dp32=dp32)
    for v in out.values():
        v.setflags(write=False)
    return out


def _cuda(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


def _run(spec, c, need_x=True, need_p=True, x=None):
    """(y, dx, d_params) of one forward + backward through texgs.mlp.fused_mlp"""
    from texgs import mlp
    xt = _cuda(c["x"], need_x) if x is None else x
    pt = _cuda(c["params"], need_p)
    y = mlp.fused_mlp(xt, pt, *spec)
    if need_x or need_p:
        y.backward(_cuda(c["dy"]))
    return y.detach(), xt.grad, pt.grad


def _within(name, got, f64, f32):
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - f64).max())
    tol = R.tolerance(f64, f32)
    print(f"{name}: max|hip - f64| {err:.3e}, bound {tol:.3e}, ratio to the cpu_f32 error (bound 4) {4 * err / tol:.2f}")
    assert err <= tol, (name, err, tol)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ---- parity against float64 ----
@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("spec", SPECS, ids=_id)
def test_forward_matches_float64(spec, k):
    from texgs import mlp
    N = _sizes(mlp.FORWARD_TILE)[k]
    c = _case(spec, N)
    y, _, _ = _run(spec, c, False, False)
    assert y.shape == (N, spec[1]) and y.dtype == torch.float32
    _within(f"y {spec} N={N}", y, c["y64"], c["y32"])


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("spec", SPECS, ids=_id)
def test_backward_matches_float64(spec, k):
    from texgs import mlp
    N = _sizes(mlp.BACKWARD_TILE)[k]
    c = _case(spec, N)
    _, dx, dp = _run(spec, c)
    assert dx.shape == (N, spec[0]) and dp.shape == (R.param_count(spec),)
    _within(f"dx {spec} N={N}", dx, c["dx64"], c["dx32"])
    _within(f"d_params {spec} N={N}", dp, c["dp64"], c["dp32"])


def test_backward_second_tile_of_a_workgroup_and_partial_last_tile():
    from texgs import mlp
    spec = (128, 128, 2)
    N = mlp.BACKWARD_TILE * mlp.BACKWARD_MAX_WORKGROUPS + mlp.BACKWARD_TILE + 1
    c = _case(spec, N)
    y, dx, dp = _run(spec, c)
    _within(f"y {spec} N={N}", y, c["y64"], c["y32"])
    _within(f"dx {spec} N={N}", dx, c["dx64"], c["dx32"])
    _within(f"d_params {spec} N={N}", dp, c["dp64"], c["dp32"])


def test_empty_batch_launches_nothing_and_zeroes_d_params():
    from texgs import mlp
    spec = (3, 128, 1)
    x = torch.empty(0, 3, device="cuda", requires_grad=True)
    p = _cuda(R.xavier_params(spec, 1), True)
    y = mlp.fused_mlp(x, p, *spec)
    assert y.shape == (0, 128)
    y.backward(torch.empty(0, 128, device="cuda"))
    assert x.grad.shape == (0, 3) and p.grad.shape == p.shape and not bool(p.grad.any())


# ---- selection, determinism, padded regions ----
@pytest.mark.parametrize("spec", [(3, 128, 1), (128, 3, 2)], ids=_id)
def test_output_selection_leaves_the_selected_gradient_unchanged(spec):
    from texgs import mlp
    c = _case(spec, 2 * mlp.BACKWARD_TILE + 1)
    y, dx, dp = _run(spec, c)
    y1, dx1, dp1 = _run(spec, c, True, False)
    y2, dx2, dp2 = _run(spec, c, False, True)
    y3, dx3, dp3 = _run(spec, c, False, False)
    assert dp1 is None and dx2 is None and dx3 is None and dp3 is None
    assert np.array_equal(_bits(dx1), _bits(dx)) and np.array_equal(_bits(dp2), _bits(dp))
    for other in (y1, y2, y3):
        assert np.array_equal(_bits(other), _bits(y))
    assert not mlp.fused_mlp(_cuda(c["x"]), _cuda(c["params"]), *spec).requires_grad


def test_backward_is_deterministic():
    from texgs import mlp
    spec = (32, 128, 1)
    c = _case(spec, 2 * mlp.BACKWARD_TILE + 1)
    a, b = _run(spec, c), _run(spec, c)
    assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    spec = (128, 128, 2)                    # every workgroup of the persistent grid and the reduce over all of them
    c = _case(spec, mlp.BACKWARD_TILE * mlp.BACKWARD_MAX_WORKGROUPS + mlp.BACKWARD_TILE + 1)
    assert np.array_equal(_bits(_run(spec, c)[2]), _bits(_run(spec, c)[2]))


@pytest.mark.parametrize("spec", [(3, 128, 1), (128, 3, 2), (17, 33, 2), (1, 1, 2)], ids=_id)
def test_padded_regions_of_d_params(spec):
    from texgs import mlp
    n_in, n_out, _ = spec
    c = _case(spec, mlp.BACKWARD_TILE + 1)
    dp = _run(spec, c)[2].cpu().numpy()
    mats = R.split(dp, spec)
    rows_padded, cols_padded = mats[-1].shape[0] > n_out, mats[0].shape[1] > n_in
    assert (rows_padded, cols_padded) == (n_out % 16 != 0, n_in % 16 != 0) and (rows_padded or cols_padded)
    assert mats[-1][:n_out].any() and mats[0][:, :n_in].any()
    if rows_padded:
        assert not mats[-1][n_out:].view(np.int32).any()          # exactly +0.0
    if cols_padded:
        pad = mats[0][:, n_in:].view(np.int32)
        assert pad.shape[1] >= 2 and (pad == pad[:, :1]).all() and pad.any()


# ---- inputs and streams ----
def test_non_contiguous_and_offset_inputs_give_the_contiguous_result():
    from texgs import mlp
    spec = (3, 128, 1)
    c = _case(spec, mlp.FORWARD_TILE + 1)
    N = c["x"].shape[0]
    want = _run(spec, c)
    wide = torch.zeros(N, 6, device="cuda")
    wide[:, ::2] = _cuda(c["x"])
    strided = wide[:, ::2].requires_grad_(True)
    assert not strided.is_contiguous()
    flat = torch.zeros(3 * N + 1, device="cuda")
    flat[1:] = _cuda(c["x"]).reshape(-1)
    shifted = flat[1:].view(N, 3)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    shifted.requires_grad_(True)
    dbl = _cuda(c["x"]).double().requires_grad_(True)                # (float32 values: the copy is exact)
    for x in (strided, shifted, dbl):
        got = _run(spec, c, x=x)
        for g, w in zip(got, want):
            assert np.array_equal(_bits(g.float()), _bits(w))
    assert dbl.grad.dtype == torch.float64


def test_side_stream_gives_the_same_bits():
    from texgs import mlp
    spec = (128, 3, 2)
    c = _case(spec, 2 * mlp.BACKWARD_TILE + 1)
    want = _run(spec, c)
    xt, pt, dy = _cuda(c["x"], True), _cuda(c["params"], True), _cuda(c["dy"])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = mlp.fused_mlp(xt, pt, *spec)
        y.backward(dy)
    s.synchronize()                         # nothing beyond the stream's own work
    for g, w in zip((y, xt.grad, pt.grad), want):
        assert np.array_equal(_bits(g), _bits(w))


def test_module_runs_and_trains():
    from texgs import mlp
    net = mlp.FusedMLP(3, 128, 1).cuda()
    assert [k for k, _ in net.named_parameters()] == ["params"] and net.params.dtype == torch.float32
    x = torch.rand(70, 3, device="cuda") * 2 - 1
    net(x).square().mean().backward()
    assert net.params.grad is not None and bool(torch.isfinite(net.params.grad).all()) and bool(net.params.grad.any())


# ---- the reference's model classes, restated (models/modules/utils.py:5-41, models/modules/uv_net.py) on the drop-in ----
def _build_tcnn_network(hash_grid, in_dims, out_dims, depth):
    """build_tcnn_network of the reference with its cfg spelled out: Sequential(Encoding, Network) with a hash grid, else a Network"""
    import tinycudann as tcnn
    if hash_grid:
        enc = tcnn.Encoding(n_input_dims=in_dims, encoding_config={
            "otype": "HashGrid", "n_levels": hash_grid["n_levels"], "n_features_per_level": hash_grid["n_features_per_level"],
            "log2_hashmap_size": hash_grid["max_hashmap"], "base_resolution": 16, "per_level_scale": 1.447})
        net = tcnn.Network(n_input_dims=hash_grid["n_levels"] * hash_grid["n_features_per_level"], n_output_dims=out_dims,
                           network_config=NETCFG(depth))
        return nn.Sequential(enc, net)
    return tcnn.Network(n_input_dims=in_dims, n_output_dims=out_dims, network_config=NETCFG(depth))


class RefUVNet(nn.Module):
    """UVNet.forward of the reference (uv_net.py:19-36) without offset / scale"""

    def __init__(self):
        super().__init__()
        self.pre_mlp = _build_tcnn_network(None, 3, 128, 1)
        self.mlp = _build_tcnn_network(None, 128, 3, 2)

    def forward(self, xyz, emb):
        x = self.pre_mlp(xyz).float()
        x = F.relu(x + emb[None, :])
        return F.normalize(self.mlp(x).float(), dim=-1)


class RefInvUVNet(nn.Module):
    """InvUVNet.forward of the reference (uv_net.py:70-85) with the shipped hash grid, without offset / scale"""

    def __init__(self):
        super().__init__()
        self.pre_mlp = _build_tcnn_network(dict(n_levels=8, n_features_per_level=4, max_hashmap=12), 3, 128, 1)
        self.mlp = _build_tcnn_network(None, 128, 3, 2)

    def forward(self, xyz, emb):
        x = self.pre_mlp(xyz / 2 + 0.5).float()
        x = F.relu(x + emb[None, :])
        return self.mlp(x).float()


def _uvnet_state(seed):
    """A tiny-cuda-nn style state of the UV net: Xavier weights, a first-layer bias in the first padded input column"""
    from texgs.uvnet import pack_tcnn_params
    g = torch.Generator().manual_seed(seed)
    u = lambda a, b: (torch.rand(a, b, generator=g) * 2 - 1) * (6.0 / (a + b)) ** 0.5
    pre = [(u(128, 3), (torch.rand(128, generator=g) - 0.5) * 0.2), (u(128, 128), None)]
    mlp = [(u(128, 128), None), (u(128, 128), None), (u(3, 128), None)]
    emb = (torch.rand(128, generator=g) - 0.5) * 0.2
    return {"pre_mlp.params": pack_tcnn_params(pre, 3, 128), "mlp.params": pack_tcnn_params(mlp, 128, 3)}, emb


def _clear_of_kinks(zs, N):
    """indices of the first N rows whose every pre-activation satisfies |z| >= 1e-3 rms(z of that layer) (mlp_ref.kink_free_inputs' rule)"""
    ok = np.ones(zs[0].shape[0], bool)
    for z in zs:
        ok &= (np.abs(z) >= 1e-3 * np.sqrt(np.mean(z * z))).all(axis=1)
    keep = np.flatnonzero(ok)[:N]
    assert keep.size == N, f"only {int(ok.sum())} candidates are clear of every kink"
    return keep


def _two_net_pre_activations(p1, spec1, p2, spec2, x, emb):
    """float64 pre-activations of net2(relu(net1(x) + emb)): the hidden layers of both nets and the sum the embedding is added to"""
    z_mid = R.forward(p1, x, spec1) + emb.astype(np.float64)
    return R.pre_activations(p1, x, spec1) + [z_mid] + R.pre_activations(p2, np.maximum(z_mid, 0), spec2)


def _tol(f64, f32):
    return R.tolerance(f64.detach().cpu().numpy(), f32.detach().cpu().numpy())


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def test_restated_uvnet_on_the_drop_in_matches_texgs_uvnet():
    from texgs.uvnet import UVNet, jacobian_by_autograd
    N = 33
    state, emb = _uvnet_state(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        shim = RefUVNet()
        shim.load_state_dict(state)
        shim = shim.cuda()
        own = UVNet(precision="fp32").load_reference_state(state)
    cand = torch.rand(2 * N, 3, generator=torch.Generator().manual_seed(4)) * 2 - 1
    zs = _two_net_pre_activations(state["pre_mlp.params"].numpy(), (3, 128, 1), state["mlp.params"].numpy(), (128, 3, 2), cand.numpy(), emb.numpy())
    xyz = cand[_clear_of_kinks(zs, N)].contiguous()
    own64 = UVNet(precision="fp32")
    own64.load_state_dict(own.state_dict())
    own64 = own64.double()
    uv64, uv32 = own64(xyz.double(), emb.double()), own(xyz, emb)                    # texgs.uvnet.UVNet, float64 and float32 on the CPU
    J64, J32 = jacobian_by_autograd(own64, xyz.double(), emb.double()), jacobian_by_autograd(own, xyz, emb)
    own = own.cuda()
    xg, eg = xyz.cuda(), emb.cuda()
    uv = shim(xg, eg)
    # the Jacobian as get_grad_uvs obtains it (models/texture_gaussian3d.py:216-227): three backward passes through the net
    jac = torch.autograd.functional.jacobian(lambda inp: shim(inp, eg).sum(dim=0), xg.detach())
    J = jac.permute(1, 0, 2).reshape(-1, 9)
    tol_uv, tol_J = _tol(uv64, uv32), _tol(J64, J32)
    e_uv, e_J = _err(uv, uv64), _err(J, J64)
    print(f"restated UVNet on the drop-in: uvs {e_uv:.3e} (bound {tol_uv:.3e}), J {e_J:.3e} (bound {tol_J:.3e})")
    assert e_uv <= tol_uv and e_J <= tol_J
    # the project's own evaluations of the same state: forward (torch on the GPU) and the fused kernel.  Each is another fp32 evaluation
    # of the function the drop-in was just held to, so two of them differ by at most two bounds.
    uv_t = own(xg, eg)
    uv_k, J_k = own.uv_and_jacobian(xg, eg)
    print(f"  against UVNet.forward {_err(uv, uv_t):.3e}, against uv_and_jacobian uvs {_err(uv, uv_k):.3e} J {_err(J, J_k):.3e}")
    assert _err(uv, uv_t) <= 2 * tol_uv and _err(uv, uv_k) <= 2 * tol_uv and _err(J, J_k) <= 2 * tol_J


def test_restated_inv_uvnet_on_the_drop_in_matches_texgs_inv_uvnet():
    """Values and the gradients to every parameter and to the input.  Both nets run the SAME hash-grid kernels, so the encoding is the same
    bits and the float64 statement starts from it: out and the MLP gradients are held to the file's bound against mlp_ref; the hash
    grid's backward is linear in d_enc with non-negative weights for its table, so two evaluations whose d_enc are each within `t` of
    the float64 one differ in d_table by at most that backward applied to the constant 2 t -- and in d_uv by at most 2 t times the
    summed |d enc / d uv|."""
    from texgs.uvmap import InvUVNet, hashgrid_encode
    N = 65
    g = torch.Generator().manual_seed(9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        shim = RefInvUVNet()
        assert list(shim.state_dict()) == ["pre_mlp.0.params", "pre_mlp.1.params", "mlp.params"]
        state = {k: v.clone() for k, v in shim.state_dict().items()}
        state["pre_mlp.0.params"] = (torch.rand(state["pre_mlp.0.params"].shape, generator=g) - 0.5) * 0.5      # (a table with signal)
        shim.load_state_dict(state)
        shim = shim.cuda()
        own = InvUVNet().load_reference_state(state).cuda()
    emb = ((torch.rand(128, generator=g) - 0.5) * 0.2).cuda()
    spec1, spec2 = (32, 128, 1), (128, 3, 2)
    cand = F.normalize(torch.randn(2 * N, 3, generator=g), dim=-1).cuda()
    enc_c = hashgrid_encode(cand / 2 + 0.5, state["pre_mlp.0.params"].cuda()).cpu().numpy()
    zs = _two_net_pre_activations(state["pre_mlp.1.params"].numpy(), spec1, state["mlp.params"].numpy(), spec2, enc_c, emb.cpu().numpy())
    uv = cand[torch.from_numpy(_clear_of_kinks(zs, N)).cuda()].contiguous()
    w = torch.randn(N, 3, generator=g).cuda()

    def grads(net, names):
        u = uv.clone().requires_grad_(True)
        out = net(u, emb)
        ps = [dict(net.named_parameters())[n] for n in names]
        gs = torch.autograd.grad((out * w).sum(), [u] + ps)
        return out.detach(), gs[0], gs[1:]

    out_s, duv_s, (dtab_s, dp1_s, dp2_s) = grads(shim, ["pre_mlp.0.params", "pre_mlp.1.params", "mlp.params"])
    out_o, duv_o, own_g = grads(own, ["encoding.params"] + [f"pre_mlp.{k}.weight" for k in (0, 2)] + [f"mlp.{k}.weight" for k in (0, 2, 4)])
    # ---- float64 and float32 statements from the shared encoding
    enc = hashgrid_encode((uv / 2 + 0.5), state["pre_mlp.0.params"].cuda()).cpu().numpy()
    p1, p2 = state["pre_mlp.1.params"].numpy(), state["mlp.params"].numpy()
    e, wn = emb.cpu().numpy(), w.cpu().numpy()

    def chain(fp32):
        dt = np.float32 if fp32 else np.float64
        a = np.maximum(R.forward(p1, enc, spec1, fp32) + e.astype(dt), 0)
        out = R.forward(p2, a, spec2, fp32)
        da, dp2 = R.backward(p2, a, wn, spec2, fp32)
        denc, dp1 = R.backward(p1, enc, da * (a > 0), spec1, fp32)
        return a, out, dp1, dp2, denc
    _, out64, dp1_64, dp2_64, denc64 = chain(False)
    _, out32, dp1_32, dp2_32, denc32 = chain(True)
    for name, got, f64, f32 in (("out", out_s, out64, out32), ("d pre_mlp.1.params", dp1_s, dp1_64, dp1_32), ("d mlp.params", dp2_s, dp2_64, dp2_32)):
        _within("restated InvUVNet " + name, got, f64, f32)
    # the project's own net holds the same weights as nn.Linear matrices: its gradients are the unpadded blocks of the flat ones
    m1, m2 = R.split(dp1_s.cpu().numpy(), spec1), R.split(dp2_s.cpu().numpy(), spec2)
    blocks = [m1[0], m1[1], m2[0], m2[1], m2[2][:3]]
    blocks64 = R.split(dp1_64, spec1) + R.split(dp2_64, spec2)
    blocks32 = R.split(dp1_32, spec1) + R.split(dp2_32, spec2)
    blocks64[-1], blocks32[-1] = blocks64[-1][:3], blocks32[-1][:3]
    for k, (b, o) in enumerate(zip(blocks, own_g[1:])):
        assert _err(torch.from_numpy(b), o) <= 2 * R.tolerance(blocks64[k], blocks32[k]), k
    assert _err(out_s, out_o) <= 2 * R.tolerance(out64, out32)
    # ---- the gradients that pass through the hash grid's backward
    t = R.tolerance(denc64, denc32)
    x01 = (uv / 2 + 0.5).detach().requires_grad_(True)
    table = state["pre_mlp.0.params"].cuda().requires_grad_(True)
    bound_tab, = torch.autograd.grad(hashgrid_encode(x01, table), table, torch.full((N, 32), 2 * t, device="cuda"))
    jac = torch.autograd.functional.jacobian(lambda x: hashgrid_encode(x, table.detach()).sum(dim=0), x01.detach())       # [32, N, 3]
    bound_uv = 2 * t * 0.5 * jac.abs().sum(dim=0)
    dtab_o = own_g[0]
    # (the table's gradient is a scatter of atomic adds whose order is free: 8 units of 2^-23 of the tensor's scale for that)
    floor_tab, floor_uv = 2.0 ** -20 * float(dtab_o.abs().max()), 2.0 ** -20 * float(duv_o.abs().max())
    print(f"restated InvUVNet: d table differs by {_err(dtab_s, dtab_o):.3e} (largest bound {float(bound_tab.max()):.3e}), "
          f"d uv by {_err(duv_s, duv_o):.3e} (largest bound {float(bound_uv.max()):.3e})")
    assert bool(((dtab_s - dtab_o).abs() <= bound_tab + floor_tab).all())
    assert bool(((duv_s - duv_o).abs() <= bound_uv + floor_uv).all())
    assert bool(dtab_s.any()) and bool(duv_s.any())


# ---- pytorch3d drop-in ----
def test_pytorch3d_drop_in_returns_the_texgs_results_bit_for_bit():
    from pytorch3d.loss import chamfer_distance
    from pytorch3d.ops import sample_farthest_points
    from texgs import points, uvmap
    g = torch.Generator().manual_seed(2)
    P, Q, K = 257, 129, 17
    x, y = torch.randn(1, P, 3, generator=g).cuda(), torch.randn(1, Q, 3, generator=g).cuda()
    for single in (False, True):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        got, none = chamfer_distance(xa, y, single_directional=single)
        want, _ = uvmap.chamfer_distance(xb, y, single_directional=single)
        assert none is None and np.array_equal(_bits(got), _bits(want))
        got.backward(); want.backward()
        assert np.array_equal(_bits(xa.grad), _bits(xb.grad))
    pts, idx = sample_farthest_points(x, K=K)
    wp, wi = points.sample_farthest_points(x[0], K, 0)
    assert pts.shape == (1, K, 3) and idx.shape == (1, K) and idx.dtype == torch.int64
    assert np.array_equal(_bits(pts[0]), _bits(wp)) and torch.equal(idx[0], wi)
