"""-m "not gpu": the fused MLP and the tinycudann / pytorch3d drop-ins without a GPU.

* The statement (tests/mlp_ref.py) against the nn.Linear evaluation of texgs.uvnet.unpack_tcnn_params: the ones-padding IS the bias
  convention the project already states.
* Structure: the ctypes mirror against gcc's layout of TexGSMlp, the header as plain C99, the exports and their signatures against the
  prototypes, texgs_mlp_param_count and the C entries' refusals (they need no GPU).
* Every refusal of texgs.mlp, tinycudann and pytorch3d is raised before any launch, by name; the drop-ins import without a GPU; the
  state-dict keys of the reference's build_tcnn_network pattern (models/modules/utils.py:5-41, restated here)."""
import ctypes as C
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import mlp_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_mlp.h")
NETCFG = lambda depth=1, **kw: {**{"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 128,
                                   "n_hidden_layers": depth}, **kw}
GRIDCFG = lambda **kw: {**{"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 4, "log2_hashmap_size": 12, "base_resolution": 16,
                           "per_level_scale": 1.447}, **kw}


@pytest.fixture(autouse=True)
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


# ---- the statement ----
@pytest.mark.parametrize("spec", [(3, 128, 1), (32, 128, 1), (128, 3, 2)])
def test_statement_is_the_linear_evaluation_of_unpack_tcnn_params(spec):
    from texgs.uvnet import unpack_tcnn_params
    n_in, n_out, L = spec
    params = R.xavier_params(spec, 3)
    # unpack_tcnn_params adds the padded columns' weights up in float32: put them on a 2^-10 grid, where that sum is exact
    pad = R.split(params, spec)[0][:, n_in:]
    pad[...] = np.round(pad * 1024) / 1024
    x = np.random.default_rng(4).uniform(-1, 1, (37, n_in))
    h = torch.from_numpy(x)
    layers = unpack_tcnn_params(torch.from_numpy(params), n_in, n_out, L)
    assert len(layers) == L + 1 and (layers[0][1] is not None) == (n_in % 16 != 0)
    for k, (w, b) in enumerate(layers):
        lin = nn.Linear(w.shape[1], w.shape[0], bias=b is not None).double()
        with torch.no_grad():
            lin.weight.copy_(w)
            if b is not None:
                lin.bias.copy_(b)
        h = lin(h)
        if k < L:
            h = torch.relu(h)
    got = R.forward(params, x, spec)
    assert got.shape == (37, n_out) and np.abs(got - h.detach().numpy()).max() <= 1e-12


def test_statement_backward_is_autograd_of_its_forward():
    spec = (17, 33, 2)
    params, x = R.kink_free_inputs(spec, 9, seed=2)
    dy = np.random.default_rng(1).standard_normal((9, 33))
    pt, xt = torch.from_numpy(params).double().requires_grad_(True), torch.from_numpy(x).double().requires_grad_(True)
    mats = R.split(pt, spec)
    h = torch.cat([xt, torch.ones(9, 32 - 17, dtype=torch.float64)], dim=1)
    for W in mats[:-1]:
        h = torch.relu(h @ W.t())
    y = (h @ mats[-1].t())[:, :33]
    assert np.abs(y.detach().numpy() - R.forward(params, x, spec)).max() <= 1e-12
    y.backward(torch.from_numpy(dy))
    dx, dp = R.backward(params, x, dy, spec)
    assert np.abs(dx - xt.grad.numpy()).max() <= 1e-12 and np.abs(dp - pt.grad.numpy()).max() <= 1e-12
    f32 = R.backward(params, x, dy, spec, fp32=True)
    assert f32[0].dtype == np.float32 and f32[1].dtype == np.float32 and 0 < np.abs(f32[1] - dp).max() < 1e-4


def test_kink_free_inputs_finds_its_points_at_the_sizes_the_gpu_tests_use():
    for spec in [(3, 128, 1), (128, 128, 2), (1, 1, 2)]:
        params, x = R.kink_free_inputs(spec, 257, seed=5)
        assert x.shape == (257, spec[0]) and x.dtype == np.float32 and params.size == R.param_count(spec)
        for z in R.pre_activations(params, x, spec):
            assert (np.abs(z) >= 1e-3 * np.sqrt(np.mean(z * z)) * 0.5).all()           # (the rms here is of the kept rows only)


# ---- structure ----
def test_struct_matches_c_layout(tmp_path):
    from texgs import mlp
    cls = mlp.MlpStruct
    consts = {"TEXGS_MLP_WIDTH": mlp.WIDTH, "TEXGS_MLP_MAX_HIDDEN_LAYERS": mlp.MAX_HIDDEN_LAYERS, "TEXGS_MLP_FORWARD_TILE": mlp.FORWARD_TILE,
              "TEXGS_MLP_BACKWARD_TILE": mlp.BACKWARD_TILE, "TEXGS_MLP_BACKWARD_MAX_WORKGROUPS": mlp.BACKWARD_MAX_WORKGROUPS}
    assert abi_check.layout_mismatches("texgs_mlp.h", {"TexGSMlp": cls}, consts, tmp_path) == []
    assert C.sizeof(cls) == 16 and [f for f, _ in cls._fields_] == ["n_in", "n_out", "n_hidden_layers", "n_neurons"]


def test_header_is_plain_c99_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_mlp.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]
    assert '#include "texgs_mlp.h"' in open(os.path.join(ROOT, "texture-gs_amd", "csrc", "mlp.hip")).read()


def test_library_exports_the_entries_and_the_signatures_match_the_prototypes(lib_built):
    from texgs import _lib, mlp
    protos = abi_check.prototypes(HDR)
    assert sorted(protos) == sorted(mlp.SIGNATURES) == sorted(["texgs_mlp_param_count", "texgs_mlp_forward_temp_bytes", "texgs_mlp_forward",
                                                                "texgs_mlp_backward_temp_bytes", "texgs_mlp_backward"])
    raw = C.CDLL(lib_built)
    assert all(hasattr(raw, name) for name in protos)
    assert abi_check.signature_mismatches(HDR, mlp.SIGNATURES, {"TexGSMlp": mlp.MlpStruct}) == []
    lib = mlp.entry()
    assert lib is _lib.load() and lib.texgs_mlp_forward.argtypes == mlp.SIGNATURES["texgs_mlp_forward"][1]
    # the mirror and the signatures live in texgs/mlp.py, not in the table that tests/test_abi.py pins to texgs.h
    assert not any(n in _lib.SIGNATURES for n in protos) and not hasattr(_lib, "MlpStruct")
    # the build knows the header: it is a dependency of every unit and part of the build id
    build = abi_check.build_knows_header(HDR)
    assert "mlp.hip" in build.UNITS


def test_param_count_and_the_c_refusals_need_no_gpu(lib_built):
    from texgs import mlp
    lib = mlp.entry()
    st = lambda *a: C.byref(mlp.MlpStruct(*a))
    for spec, want in [((3, 128, 1), 128 * 16 + 128 * 128), ((32, 128, 1), 128 * 32 + 128 * 128), ((128, 3, 2), 2 * 128 * 128 + 16 * 128),
                       ((128, 128, 2), 3 * 128 * 128), ((17, 33, 2), 128 * 32 + 128 * 128 + 48 * 128)]:
        assert lib.texgs_mlp_param_count(st(*spec, 128)) == want == R.param_count(spec) == mlp.param_count(*spec)
        assert lib.texgs_mlp_forward_temp_bytes(st(*spec, 128), 1000) > 0
        assert lib.texgs_mlp_backward_temp_bytes(st(*spec, 128), 1000) > lib.texgs_mlp_backward_temp_bytes(st(*spec, 128), 1)
    buf = (C.c_float * 64)()                # stands in for device memory: a refused call reads nothing
    b = (C.addressof(buf) + 15) // 16 * 16

    def refused(fields, cause):
        assert lib.texgs_num_rendered_reduce(None, 4, None, None) != 0 and cause.encode() not in lib.texgs_last_error()      # another message first
        assert lib.texgs_mlp_param_count(st(*fields)) == 0
        assert cause.encode() in lib.texgs_last_error(), (cause, lib.texgs_last_error())
        assert lib.texgs_mlp_forward_temp_bytes(st(*fields), 10) == 0 and lib.texgs_mlp_backward_temp_bytes(st(*fields), 10) == 0
        assert lib.texgs_mlp_forward(st(*fields), b, b, 4, b, b, None) != 0
        assert lib.texgs_mlp_backward(st(*fields), b, b, b, 4, b, b, b, None) != 0
        assert cause.encode() in lib.texgs_last_error()

    refused((3, 128, 1, 64), "n_neurons must be 128, got 64")
    refused((3, 128, 0, 128), "n_hidden_layers must be 1 or 2, got 0")
    refused((3, 128, 3, 128), "n_hidden_layers must be 1 or 2, got 3")
    refused((0, 128, 1, 128), "n_in must be in [1,128], got 0")
    refused((129, 128, 1, 128), "n_in must be in [1,128], got 129")
    refused((3, 0, 1, 128), "n_out must be in [1,128], got 0")
    refused((3, 129, 1, 128), "n_out must be in [1,128], got 129")
    good = st(3, 128, 1, 128)
    for call, cause in [(lambda: lib.texgs_mlp_forward(None, b, b, 4, b, b, None), "mlp is NULL"),
                        (lambda: lib.texgs_mlp_forward(good, b, b, -1, b, b, None), "N < 0"),
                        (lambda: lib.texgs_mlp_forward(good, None, b, 4, b, b, None), "NULL argument (params or temp)"),
                        (lambda: lib.texgs_mlp_forward(good, b, b, 4, b, None, None), "NULL argument (params or temp)"),
                        (lambda: lib.texgs_mlp_forward(good, b, None, 4, b, b, None), "NULL argument (x or y)"),
                        (lambda: lib.texgs_mlp_forward(good, b + 2, b, 4, b, b, None), "params must be 4-byte aligned"),
                        (lambda: lib.texgs_mlp_forward(good, b, b, 4, b, b + 4, None), "temp must be 16-byte aligned"),
                        (lambda: lib.texgs_mlp_forward(good, b, b + 1, 4, b, b, None), "x and y must be 4-byte aligned"),
                        (lambda: lib.texgs_mlp_backward(good, b, None, b, 4, b, b, b, None), "NULL argument (x or dy)"),
                        (lambda: lib.texgs_mlp_backward(good, b, b, b, 4, b + 2, b, b, None), "x, dy, dx and d_params must be 4-byte aligned"),
                        (lambda: lib.texgs_mlp_backward(good, b, b, b, 2 ** 31 - 1, b, b, b, None), "N too large")]:
        assert call() != 0 and cause.encode() in lib.texgs_last_error(), (cause, lib.texgs_last_error())
    # N = 0 with nothing to zero: success, and nothing is launched
    assert lib.texgs_mlp_forward(good, b, None, 0, None, b, None) == 0
    assert lib.texgs_mlp_backward(good, b, None, None, 0, None, None, b, None) == 0


# ---- texgs.mlp: refusals before any launch, by name ----
def test_fused_mlp_refusals(monkeypatch):
    from texgs import mlp
    monkeypatch.setattr(mlp, "entry", lambda: pytest.fail("a refused call reached the library"))
    x, p = torch.zeros(5, 3), torch.zeros(mlp.param_count(3, 128, 1))
    with pytest.raises(NotImplementedError, match=r"n_hidden_layers = 3 is not supported"):
        mlp.fused_mlp(x, p, 3, 128, 3)
    with pytest.raises(NotImplementedError, match=r"n_hidden_layers = 0 is not supported"):
        mlp.fused_mlp(x, p, 3, 128, 0)
    with pytest.raises(NotImplementedError, match=r"n_in = 129 is not supported"):
        mlp.fused_mlp(torch.zeros(5, 129), p, 129, 128, 1)
    with pytest.raises(NotImplementedError, match=r"n_out = 0 is not supported"):
        mlp.fused_mlp(x, p, 3, 0, 1)
    with pytest.raises(NotImplementedError, match=r"n_neurons = 64 is not supported"):
        mlp.check_shape(3, 128, 1, 64)
    with pytest.raises(TypeError, match=r"n_in must be an int"):
        mlp.fused_mlp(x, p, 3.0, 128, 1)
    with pytest.raises(ValueError, match=r"x must be \[N, 3\], got \(5, 4\)"):
        mlp.fused_mlp(torch.zeros(5, 4), p, 3, 128, 1)
    with pytest.raises(ValueError, match=r"x must be \[N, 3\], got \(3,\)"):
        mlp.fused_mlp(torch.zeros(3), p, 3, 128, 1)
    with pytest.raises(ValueError, match=r"expected a flat params tensor of 18432 values .* got shape \(18431,\)"):
        mlp.fused_mlp(x, p[:-1], 3, 128, 1)
    with pytest.raises(ValueError, match=r"expected a flat params tensor of 18432 values"):
        mlp.fused_mlp(x, p.reshape(128, -1), 3, 128, 1)
    with pytest.raises(RuntimeError, match=r"x must be on an AMD GPU; there is no CPU fallback"):
        mlp.fused_mlp(x, p, 3, 128, 1)
    with pytest.raises(NotImplementedError, match=r"n_hidden_layers = 4"):
        mlp.FusedMLP(3, 128, 4)


def test_module_state_and_initialisation():
    from texgs import mlp
    a, b, c = mlp.FusedMLP(3, 128, 1), mlp.FusedMLP(3, 128, 1), mlp.FusedMLP(3, 128, 1, seed=7)
    assert list(a.state_dict()) == ["params"] and a.params.dtype == torch.float32 and a.params.shape == (18432,)
    assert torch.equal(a.params, b.params) and not torch.equal(a.params, c.params)
    for m, (rows, cols) in zip(R.split(a.params.detach().numpy(), (3, 128, 1)), [(128, 16), (128, 128)]):
        bound = (6.0 / (rows + cols)) ** 0.5
        assert m.shape == (rows, cols) and np.abs(m).max() <= bound and np.abs(m).max() > 0.9 * bound and abs(m.mean()) < 0.05 * bound
    assert "not bit-equal" in mlp.FusedMLP.__doc__.lower().replace("\n", " ")
    assert (mlp.FORWARD_TILE, mlp.BACKWARD_TILE, mlp.BACKWARD_MAX_WORKGROUPS) == (128, 64, 256)


# ---- tinycudann ----
def test_tinycudann_imports_without_a_gpu_and_refuses_by_name(lib_built):
    import tinycudann as tcnn
    net = tcnn.Network(3, 128, NETCFG())
    assert isinstance(net, nn.Module) and (net.n_input_dims, net.n_output_dims) == (3, 128) and list(net.state_dict()) == ["params"]
    assert tcnn.Network(n_input_dims=128, n_output_dims=3, network_config=NETCFG(2, otype="CutlassMLP")).params.numel() == 34816
    for kw, text in [(dict(otype="MegaMLP"), r"network otype 'MegaMLP' is not supported"), (dict(activation="Sigmoid"), r"activation 'Sigmoid'"),
                     (dict(output_activation="ReLU"), r"output_activation 'ReLU'"), (dict(n_neurons=64), r"n_neurons = 64"),
                     (dict(n_hidden_layers=3), r"n_hidden_layers = 3"), (dict(n_hidden_layers=0), r"n_hidden_layers = 0"),
                     (dict(feedback_alignment=True), r"network_config key 'feedback_alignment'")]:
        with pytest.raises(NotImplementedError, match=text):
            tcnn.Network(3, 128, NETCFG(**kw))
    with pytest.raises(NotImplementedError, match=r"n_input_dims = 200"):
        tcnn.Network(200, 3, NETCFG())
    with pytest.raises(NotImplementedError, match=r"n_output_dims = 0"):
        tcnn.Network(3, 0, NETCFG())
    with pytest.raises(NotImplementedError, match=r"NetworkWithInputEncoding is not supported"):
        tcnn.NetworkWithInputEncoding(3, 3, GRIDCFG(), NETCFG())
    enc = tcnn.Encoding(n_input_dims=3, encoding_config=GRIDCFG())
    assert enc.n_output_dims == 32 and list(enc.state_dict()) == ["params"]
    for args, text in [((3, GRIDCFG(otype="Frequency")), r"encoding otype 'Frequency'"), ((2, GRIDCFG()), r"n_input_dims = 2"),
                       ((3, GRIDCFG(interpolation="Smoothstep")), r"encoding_config key 'interpolation'"),
                       ((3, GRIDCFG(n_features_per_level=2)), r"HashGrid .* is not supported"), ((3, GRIDCFG(n_levels=17)), r"HashGrid .* is not supported")]:
        with pytest.raises(NotImplementedError, match=text):
            tcnn.Encoding(*args)
    with pytest.raises(RuntimeError, match=r"no CPU fallback"):
        net(torch.zeros(4, 3))


def test_tinycudann_warns_once_that_the_layout_is_unpinned(lib_built, monkeypatch):
    import tinycudann as tcnn
    monkeypatch.setattr(tcnn, "_warned", False)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        tcnn.Network(3, 128, NETCFG())
        tcnn.Network(3, 128, NETCFG())
    texts = [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(texts) == 1 and "UNPINNED" in texts[0]


def _build_tcnn_network(hash_grid, in_dims, out_dims, depth):
    """build_tcnn_network of the reference with its cfg spelled out"""
    import tinycudann as tcnn
    if hash_grid:
        enc = tcnn.Encoding(n_input_dims=in_dims, encoding_config={
            "otype": "HashGrid", "n_levels": hash_grid["n_levels"], "n_features_per_level": hash_grid["n_features_per_level"],
            "log2_hashmap_size": hash_grid["max_hashmap"], "base_resolution": 16, "per_level_scale": 1.447})
        net = tcnn.Network(n_input_dims=hash_grid["n_levels"] * hash_grid["n_features_per_level"], n_output_dims=out_dims,
                           network_config=NETCFG(depth))
        return nn.Sequential(enc, net)
    return tcnn.Network(n_input_dims=in_dims, n_output_dims=out_dims, network_config=NETCFG(depth))


def test_state_dict_keys_of_the_reference_pattern(lib_built):
    from texgs.uvmap import InvUVNet, hashgrid_levels

    class Inv(nn.Module):
        def __init__(self):
            super().__init__()
            self.pre_mlp = _build_tcnn_network(dict(n_levels=8, n_features_per_level=4, max_hashmap=12), 3, 128, 1)
            self.mlp = _build_tcnn_network(None, 128, 3, 2)

    class UV(nn.Module):
        def __init__(self):
            super().__init__()
            self.pre_mlp = _build_tcnn_network(None, 3, 128, 1)
            self.mlp = _build_tcnn_network(None, 128, 3, 2)

    inv, uv = Inv(), UV()
    sd = inv.state_dict()
    assert list(sd) == ["pre_mlp.0.params", "pre_mlp.1.params", "mlp.params"] and list(uv.state_dict()) == ["pre_mlp.params", "mlp.params"]
    assert [v.numel() for v in sd.values()] == [hashgrid_levels()["n_params"], 128 * 32 + 128 * 128, 2 * 128 * 128 + 16 * 128]
    assert [v.numel() for v in uv.state_dict().values()] == [128 * 16 + 128 * 128, 2 * 128 * 128 + 16 * 128]
    # a tiny-cuda-nn state (fp16 storage) loads with a plain load_state_dict, and is the state texgs.uvmap.InvUVNet reads
    half = {k: (torch.rand(v.shape) - 0.5).half() for k, v in sd.items()}
    inv.load_state_dict(half)
    assert all(v.dtype == torch.float32 and torch.equal(v, half[k].float()) for k, v in inv.state_dict().items())
    own = InvUVNet().load_reference_state(inv.state_dict())
    assert torch.equal(own.pre_mlp[0].weight, inv.pre_mlp[1].params[:128 * 32].reshape(128, 32))
    assert torch.equal(own.mlp[4].weight, inv.mlp.params[2 * 128 * 128:].reshape(16, 128)[:3])


# ---- pytorch3d ----
def test_pytorch3d_imports_without_a_gpu_and_refuses_by_name():
    import pytorch3d.loss
    import pytorch3d.ops
    from pytorch3d.loss import chamfer_distance
    from pytorch3d.ops import sample_farthest_points
    x, y = torch.zeros(1, 7, 3), torch.zeros(1, 5, 3)
    for kw, text in [(dict(x_lengths=torch.tensor([7])), r"x_lengths"), (dict(y_lengths=torch.tensor([5])), r"y_lengths"),
                     (dict(x_normals=x), r"x_normals"), (dict(y_normals=y), r"y_normals"), (dict(weights=torch.ones(1)), r"weights"),
                     (dict(batch_reduction="sum"), r"batch_reduction='sum'"), (dict(point_reduction="sum"), r"point_reduction='sum'"),
                     (dict(point_reduction=None), r"point_reduction=None"), (dict(norm=1), r"norm=1"), (dict(abs_cosine=False), r"abs_cosine=False"),
                     (dict(single_directional=1), r"single_directional=1")]:
        with pytest.raises(NotImplementedError, match=text):
            chamfer_distance(x, y, **kw)
    with pytest.raises(NotImplementedError, match=r"batch size 2"):
        chamfer_distance(torch.zeros(2, 7, 3), torch.zeros(2, 5, 3))
    with pytest.raises(RuntimeError, match=r"no CPU fallback"):
        chamfer_distance(x, y)
    for kw, text in [(dict(lengths=torch.tensor([7])), r"lengths"), (dict(random_start_point=True), r"random_start_point=True"),
                     (dict(K=[3]), r"K=\[3\]"), (dict(K=torch.tensor([3])), r"K=tensor")]:
        with pytest.raises(NotImplementedError, match=text):
            sample_farthest_points(x, **{**dict(K=3), **kw})
    with pytest.raises(NotImplementedError, match=r"batch size 2"):
        sample_farthest_points(torch.zeros(2, 7, 3), K=3)
    with pytest.raises(ValueError, match=r"points must be \[1, P, 3\]"):
        sample_farthest_points(torch.zeros(7, 3), K=3)
    with pytest.raises(RuntimeError, match=r"no CPU fallback"):
        sample_farthest_points(x, K=3)
