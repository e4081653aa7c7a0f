"""-m "not gpu": the fused Adam step without a GPU.

* The statement (tests/adam_ref.py) against torch's CPU Adam, foreach=False and foreach=True: 8 steps on 65 536 elements, the state
  taken over from torch after every step so that only one-step differences are measured, in units of 2^-24 of a scale
  (adam_ref.scaled_units).  Bounds: m' and v' <= 4 units (three roundings on each side), p' <= 16 units (seven on each side).
* Structure: the ctypes record against gcc's layout of TexGSAdamTensor, the header as plain C99, the export, the signature against
  the prototype, the C entry's refusals (they need no GPU), the Python refusals by name, and the state-dict round trip with the three
  Adam states of tests/golden/ckpt_stage3.pth."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import adam_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "texgs_optim.h")


# ---- the statement against torch's CPU Adam ----
@pytest.mark.parametrize("foreach", [False, True])
def test_statement_against_torch_cpu_adam(foreach):
    from texgs import optim  # noqa: F401  (the feature under test: the statement states ITS scalars)
    n, lr, betas, eps = 65536, 1e-2, (0.9, 0.999), 1e-15
    p_np, grad = R.parity_inputs(n, seed=1)
    p = torch.nn.Parameter(torch.from_numpy(p_np.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=foreach)
    worst = np.zeros(3)
    for k in range(8):
        g = grad(k)
        p0 = p.detach().numpy().copy()
        st = opt.state.get(p)
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros(n, np.float32)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(n, np.float32)
        (p1, m1, v1, step1), = R.step_np([(p0, g, m0, v0, k, lr, betas, eps)])
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[p]
        assert float(st["step"]) == step1
        units = R.scaled_units(p0, g, m0, v0, (p1, m1, v1), (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()))
        worst = np.maximum(worst, units)
    print(f"foreach={foreach}: statement against torch {torch.__version__} CPU Adam, units of 2^-24: p' {worst[0]:.2f}  m' {worst[1]:.2f}  "
          f"v' {worst[2]:.2f}")
    assert worst[1] <= 4.0 and worst[2] <= 4.0, worst
    assert worst[0] <= 16.0, worst


def test_scalars_are_the_statements():
    from texgs import optim
    for step, lr, betas, eps in [(1, 1e-2, (0.9, 0.999), 1e-15), (7, 1.6e-4, (0.3, 0.99), 1e-8), (40000, 2.5e-3, (0.9, 0.999), 1e-15)]:
        got, want = optim.scalars(step, lr, betas, eps), R.scalars(step, lr, betas, eps)
        assert [np.float32(x).view(np.int32) for x in got] == [x.view(np.int32) for x in want]
        assert all(isinstance(x, float) and C.c_float(x).value == x for x in got)         # already rounded to f32
    assert optim.CHUNK == 1024 and optim.MAX_TENSORS == 32


# ---- structure ----
def _defines():
    src = open(HDR).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(TEXGS_ADAM_\w+)\s+(\d+)", src)}


def test_record_matches_c_layout(tmp_path):
    from texgs import optim
    cls = optim.AdamTensor
    consts = {"TEXGS_ADAM_MAX_TENSORS": optim.MAX_TENSORS, "TEXGS_ADAM_CHUNK": optim.CHUNK}
    assert abi_check.layout_mismatches("texgs_optim.h", {"TexGSAdamTensor": cls}, consts, tmp_path) == []
    assert C.sizeof(cls) == 64
    assert [f for f, _ in cls._fields_] == ["p", "g", "m", "v", "numel", "w1", "beta2", "w2", "bc2_sqrt", "eps", "neg_step_size"]


def test_header_is_plain_c99_and_stands_alone(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "texgs_optim.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", str(src), "-o", str(tmp_path / "c.o")])
    text = open(HDR).read()
    assert sorted(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text)) == ["stddef.h", "stdint.h"]


def test_library_exports_the_entry_and_the_signature_matches_the_prototype(lib_built):
    from texgs import _lib, optim
    (name, (ret, args)), = abi_check.prototypes(HDR).items()
    assert (ret, name, args) == ("int", "texgs_adam_step", ["TexGSAdamTensor*", "int32_t", "int32_t", "void*"])
    assert hasattr(C.CDLL(lib_built), name)
    restype, argtypes = optim.SIGNATURE
    assert abi_check.signature_mismatches(HDR, {name: optim.SIGNATURE}, {"TexGSAdamTensor": optim.AdamTensor}) == []
    fn = optim.entry()
    assert fn is _lib.load().texgs_adam_step and fn.argtypes == argtypes and fn.restype is restype
    # the mirror and the signature live in texgs/optim.py, not in the table that tests/test_abi.py pins to texgs.h
    assert name not in _lib.SIGNATURES and not hasattr(_lib, "AdamTensor")


def test_a_library_without_the_symbol_is_refused_like_a_stale_one(monkeypatch):
    from texgs import _lib, optim

    class Old:
        pass
    monkeypatch.setattr(_lib, "_bound", {})             # no table counts as applied: entry() has to bind
    monkeypatch.setattr(_lib, "load", lambda: Old())
    with pytest.raises(RuntimeError, match=r"does not export texgs_adam_step; rebuild it with `python texture-gs_amd/build.py`"):
        optim.entry()


def test_c_entry_refusals_need_no_gpu(lib_built):
    from texgs import _lib, optim
    fn, lib = optim.entry(), _lib.load()
    buf = (C.c_float * 64)()                # stands in for device memory: a refused call reads nothing
    b = C.addressof(buf)
    assert b % 16 == 0 or b % 4 == 0
    good = lambda **kw: optim.AdamTensor(**{**dict(p=b, g=b + 64, m=b + 128, v=b + 192, numel=8, w1=0.1, beta2=0.999, w2=0.001,
                                                   bc2_sqrt=1.0, eps=1e-15, neg_step_size=-0.01), **kw})

    def refused(recs, count, cause):
        arr = (optim.AdamTensor * max(len(recs), 1))(*recs)
        assert lib.texgs_num_rendered_reduce(None, 4, None, None) != 0 and cause.encode() not in lib.texgs_last_error()   # another message first
        assert fn(arr, count, 0, None) != 0, cause
        assert cause.encode() in lib.texgs_last_error(), (cause, lib.texgs_last_error())

    refused([good()], -1, "count < 0")
    refused([good(numel=0), good(numel=-5)], 2, "numel < 0")
    for k in ("p", "g", "m", "v"):
        refused([good(**{k: None})], 1, "NULL pointer")
        refused([good(**{k: b + 2})], 1, "4-byte aligned")
        refused([good(numel=0, p=None, g=None, m=None, v=None)] * 40 + [good(**{k: b + 1})], 41, "4-byte aligned")   # past the first launch's table
    with pytest.raises(RuntimeError, match=r"texgs_adam_step failed \(code -1\): count < 0"):
        _lib.call(fn, (optim.AdamTensor * 1)(good()), -1, 0, None)
    # no-ops: count == 0 (with a NULL table), and records of numel == 0 whose pointers are NULL -- no launch is made for them
    assert fn(None, 0, 0, None) == 0 and fn(None, 0, 1, None) == 0
    empty = optim.AdamTensor(None, None, None, None, 0, 0.1, 0.999, 0.001, 1.0, 1e-15, -0.01)
    for count in (1, 33):
        assert fn((optim.AdamTensor * count)(*([empty] * count)), count, 1, None) == 0
    assert fn(None, 1, 0, None) != 0 and b"NULL" in lib.texgs_last_error()


def test_python_refusals_by_name():
    from texgs import optim
    w = lambda *s, **kw: torch.nn.Parameter(torch.zeros(*s, **kw))
    with pytest.raises(ValueError, match="weight_decay"):
        optim.FusedAdam([w(4)], weight_decay=0.1)
    for k in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        with pytest.raises(ValueError, match=k):
            optim.FusedAdam([w(4)], **{k: True})
    opt = optim.FusedAdam([w(4)], lr=1e-3, eps=1e-15, foreach=True)         # foreach is torch's business: accepted, ignored
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["eps"] == 1e-15
    assert opt.step() is None and len(opt.state) == 0                         # no gradient anywhere: nothing to do, no library needed
    # a group edited after construction (add_param_group, load_state_dict) is checked at step time
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    opt.param_groups[0]["amsgrad"] = False
    opt.param_groups[0]["weight_decay"] = 0.5
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()

    def stepping(p, grad, match, exc=(ValueError, RuntimeError)):
        o = optim.FusedAdam([p], lr=1e-3)
        p.grad = grad
        with pytest.raises(exc, match=match):
            o.step()
        with pytest.raises(exc, match=match):
            optim.fused_step([o])
        assert len(o.state) == 0            # raised before any state was made or any counter advanced

    p = w(4, 3)
    stepping(p, torch.ones(4, 3), "must be on an AMD GPU; there is no CPU fallback", RuntimeError)
    p = w(4, 3, dtype=torch.float64)
    stepping(p, torch.ones(4, 3, dtype=torch.float64), r"parameter 0 of group 0 must be torch.float32")
    p = w(4, 3)            # (torch itself refuses a gradient of another dtype than its parameter's)
    stepping(p, torch.ones(3, 4).t(),r"the gradient of parameter 0 of group 0 must be contiguous")
    stepping(p, torch.ones(4, 3).to_sparse(), "sparse")
    p = torch.nn.Parameter(torch.zeros(3, 4).t())
    stepping(p, torch.ones(4, 3), r"parameter 0 of group 0 must be contiguous")
    with pytest.raises(TypeError, match="FusedAdam instances"):
        optim.fused_step([torch.optim.Adam([w(2)])])
    # a moment of the wrong kind (a state loaded from elsewhere) is named too
    p = w(4)
    o = optim.FusedAdam([p])
    p.grad = torch.ones(4)
    o.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.zeros(4, dtype=torch.float64), "exp_avg_sq": torch.zeros(4)}
    with pytest.raises(ValueError, match="exp_avg of parameter 0 of group 0 must be torch.float32"):
        o.step()
    assert float(o.state[p]["step"]) == 3.0


def _same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"])
    for k in a["state"]:
        assert sorted(a["state"][k]) == sorted(b["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.dtype == y.dtype and x.device == y.device and x.shape == y.shape and torch.equal(x, y), (k, name)


def test_state_dict_round_trip_with_the_reference_checkpoint():
    """The three Adam states the reference wrote (setup_optim + one step + state_dict, tests/golden/ckpt_stage3.pth) load into
    FusedAdam, come back unchanged, and a FusedAdam's state_dict loads into a plain torch.optim.Adam."""
    from texgs import optim, texture_io
    st = texture_io.load_checkpoint(os.path.join(ROOT, "tests", "golden", "ckpt_stage3.pth"))
    states = [s for s in st.optim_state if isinstance(s, dict) and "param_groups" in s]
    assert len(states) == 3
    for sd in states:
        def fresh(cls):
            groups = []
            for g in sd["param_groups"]:
                ps = [torch.nn.Parameter(torch.zeros(sd["state"][i]["exp_avg"].shape)) for i in g["params"]]
                groups.append({"params": ps, **({"name": g["name"]} if "name" in g else {})})
            return cls(groups, lr=0.0, eps=1e-15)
        fused = fresh(optim.FusedAdam)
        fused.load_state_dict(sd)
        back = fused.state_dict()
        _same_state_dict(back, sd)
        for s in fused.state.values():
            assert s["step"].device.type == "cpu" and s["step"].dtype == torch.float32 and float(s["step"]) == 1.0
        plain = fresh(torch.optim.Adam)
        plain.load_state_dict(back)
        _same_state_dict(plain.state_dict(), sd)
        for p in (q for g in plain.param_groups for q in g["params"]):       # and torch steps what FusedAdam handed over
            p.grad = torch.ones_like(p)
        plain.step()
        assert all(float(s["step"]) == 2.0 for s in plain.state.values())
