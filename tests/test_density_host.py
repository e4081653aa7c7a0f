"""-m "not gpu": the statement of stage-1 density control (tests/density_ref.py) against the reference's own functions through
tests/golden/density.npz, the argument checks of texgs.density, and the new entries of the C ABI.

Tolerances (computed values against the golden, which torch computed on a CPU): children's scaling 2e-6 absolute (expf, one division,
logf, each within 1 ulp, on values below 8); children's xyz 2e-6 absolute (about ten fp32 operations on terms within +-4); accumulated
norms 1e-6 relative (torch's CPU norm accumulates in double).  Everything copied is compared for equality."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import density_ref as R  # noqa: E402

GOLD = R.golden()
TOL_NORM = R.TOL_NORM
golden_case, check_against_golden = R.golden_case, R.check_against_golden


@pytest.mark.parametrize("tag", ["sh3", "sh1"])
def test_statement_reproduces_the_reference_densify_and_prune(tag):
    params, moments, accum, denom = golden_case(tag)
    max_grad, min_opacity, extent, max_screen_size, percent_dense = GOLD[f"{tag}_settings"]
    action, rank, totals = R.plan_np(accum, denom, params["scaling"], params["opacity"], max_grad, min_opacity, percent_dense * extent,
                                     0.1 * extent, densify=True, use_big=bool(max_screen_size))
    eps = GOLD[f"{tag}_eps"]
    assert eps.shape == (2 * totals[2], 3)
    got, got_m = R.move_np(params, moments, action, rank, totals, eps)
    n_out = GOLD[f"{tag}_out_xyz"].shape[0]
    assert totals[0] + totals[1] + 2 * totals[3] == n_out
    check_against_golden(tag, got, got_m, int(totals[0] + totals[1]), tag)
    # every class of the fixture is there, and the returned state is all zeros at the new size
    counts = dict(zip(["clones", "pruned clones", "split", "split pruned", "pruned originals", "denom0"], GOLD[f"{tag}_class_counts"]))
    assert totals[1] == counts["clones"] and totals[3] == counts["split"] and totals[2] == counts["split"] + counts["split pruned"]
    assert int(((action & R.CLONE) != 0).sum()) == counts["clones"] + counts["pruned clones"]
    assert min(counts.values()) >= 4
    for k in ("accum", "denom", "max_radii2D"):
        assert GOLD[f"{tag}_out_{k}"].shape[0] == n_out and not GOLD[f"{tag}_out_{k}"].any()
    assert (GOLD[f"{tag}_in_max_radii2D"] > 20).sum() >= 4          # max_radii2D above max_screen_size pruned nothing
    for k in R.GROUPS:
        assert GOLD[f"{tag}_out_{k}_step"] == GOLD[f"{tag}_in_{k}_step"] == 1.0


def test_max_screen_size_only_switches_the_world_size_prune():
    """sh1 ran without max_screen_size: Gaussians larger than 0.1 extent survive there, and go when the switch is on."""
    params, _, accum, denom = golden_case("sh1")
    max_grad, min_opacity, extent, _, percent_dense = GOLD["sh1_settings"]
    a = [R.plan_np(accum, denom, params["scaling"], params["opacity"], max_grad, min_opacity, percent_dense * extent, 0.1 * extent,
                   use_big=u)[2] for u in (False, True)]
    assert a[0][0] > a[1][0] and a[0][3] > a[1][3] and a[0][2] == a[1][2]


def test_statement_reproduces_the_reference_opacity_prune():
    params, moments, accum, denom = golden_case("prune")
    action, rank, totals = R.plan_np(accum, denom, params["scaling"], params["opacity"], 1.0, float(GOLD["prune_min_opacity"]), 0.0, 0.0,
                                     densify=False, use_big=False)
    assert totals[1] == totals[2] == totals[3] == 0 and 0 < totals[0] < len(action)
    got, got_m = R.move_np(params, moments, action, rank, totals, None)
    check_against_golden("prune", got, got_m, int(totals[0]))
    kept = np.flatnonzero(action & R.KEEP)
    for k in ("accum", "denom", "max_radii2D"):         # prune_points masks the statistics, it does not zero them
        assert np.array_equal(GOLD[f"prune_in_{k}"][kept], GOLD[f"prune_out_{k}"])


def test_statement_reproduces_the_reference_resets():
    got = R.reset_opacity_np(GOLD["reset_in_opacity"])
    assert np.abs(got.astype(np.float64) - GOLD["reset_out_opacity"]).max() <= 2e-6
    assert np.array_equal(R.reset_min_scale_np(GOLD["reset_in_scaling"]), GOLD["reset_out_scaling"])


def test_statement_reproduces_the_reference_statistics():
    n = GOLD["stats_radii0"].shape[0]
    state = (np.zeros((n, 1), np.float32), np.zeros((n, 1), np.float32), np.zeros(n, np.float32))
    for r in range(2):
        state = R.stats_np(*state, GOLD[f"stats_grad{r}"], GOLD[f"stats_radii{r}"])
        want = GOLD[f"stats_accum{r}"].astype(np.float64)
        rel = np.abs(state[0].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-30)
        assert rel.max() <= TOL_NORM, rel.max()
        assert np.array_equal(state[1], GOLD[f"stats_denom{r}"])
        assert np.array_equal(state[2], GOLD[f"stats_max_radii2D{r}"])
        assert np.array_equal(state[0] == 0, want == 0)


def test_plan_by_hand():
    """Six Gaussians, one of each fate, thresholds max_grad 1, min_opacity 0.5, dense 1, big 10."""
    ln = np.log
    scaling = np.array([[ln(.5)] * 3, [ln(.5)] * 3, [ln(2.)] * 3, [ln(2.)] * 3, [ln(20.)] * 3, [ln(.5)] * 3], np.float32)
    opacity = np.array([[2.], [2.], [2.], [-2.], [2.], [-2.]], np.float32)
    accum = np.array([[0.], [6.], [6.], [6.], [6.], [6.]], np.float32)
    denom = np.array([[0.], [2.], [2.], [2.], [2.], [2.]], np.float32)
    action, rank, totals = R.plan_np(accum, denom, scaling, opacity, 1.0, 0.5, 1.0, 10.0)
    K, C, CK, S, CH = R.KEEP, R.CLONE, R.CLONE_KEPT, R.SPLIT, R.CHILD
    #            0/0 -> g 0   clone        split      split, low op   split, child 12.5 > 10   clone, low op
    assert action.tolist() == [K, K | C | CK, S | CH, S, S, C]
    assert totals.tolist() == [2, 1, 3, 1]
    assert rank.tolist() == [[0, 1, 2, 2, 2, 2], [0, 0, 1, 1, 1, 1], [0, 0, 0, 1, 2, 3], [0, 0, 0, 1, 1, 1]]
    params = {"xyz": np.arange(18, dtype=np.float32).reshape(6, 3), "f_dc": np.zeros((6, 1, 3), np.float32),
              "f_rest": np.zeros((6, 3, 3), np.float32), "opacity": opacity, "scaling": scaling,
              "rotation": np.tile(np.array([2., 0, 0, 0], np.float32), (6, 1))}
    noise = np.zeros((6, 3), np.float32)
    noise[0], noise[3] = [1, 0, 0], [0, 1, 0]               # child 0 and child 1 of split parent j = 0 (Gaussian 2)
    out, _ = R.move_np(params, {}, action, rank, totals, noise)
    assert out["xyz"].tolist() == [[0, 1, 2], [3, 4, 5], [3, 4, 5], [8, 7, 8], [6, 9, 8]]       # identity rotation, s = 2
    assert np.allclose(out["scaling"][3:], ln(2. / 1.6), atol=1e-6) and np.array_equal(out["scaling"][:3], scaling[[0, 1, 1]])


def _model(n=16, device="cpu"):
    g = torch.Generator().manual_seed(0)
    shapes = {"xyz": (n, 3), "f_dc": (n, 1, 3), "f_rest": (n, 15, 3), "opacity": (n, 1), "scaling": (n, 3), "rotation": (n, 4)}
    params = {k: torch.nn.Parameter(torch.randn(*s, generator=g).to(device)) for k, s in shapes.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    return params, opt


def test_arguments_are_checked_before_any_library_call(lib_built, monkeypatch):
    from texgs import _lib, density

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_launch)
    n = 16
    kw = dict(max_grad=0.0002, min_opacity=0.005, extent=1.0, max_screen_size=20, percent_dense=0.01)
    st = density.DensityState.zeros(n, "cpu")
    params, opt = _model(n)
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        density.add_densification_stats(st, torch.zeros(n, 3), torch.zeros(n, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        density.densify_and_prune(params, opt, st, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        density.opacity_prune(params, opt, st, 0.005)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        density.reset_opacity(params, opt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        density.reset_min_scale(params, opt)
    # shapes and dtypes of the statistics
    with pytest.raises(ValueError, match=r"viewspace_grad must be \[N, 3\]"):
        density.add_densification_stats(st, torch.zeros(n, 2), torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match="radii must be torch.int32"):
        density.add_densification_stats(st, torch.zeros(n, 3), torch.zeros(n, dtype=torch.int64))
    with pytest.raises(ValueError, match="viewspace_grad must be torch.float32"):
        density.add_densification_stats(st, torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match="radii holds 15 rows"):
        density.add_densification_stats(st, torch.zeros(n, 3), torch.zeros(n - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"xyz_gradient_accum must be \[N, 1\]"):
        density.add_densification_stats(density.DensityState(torch.zeros(n), torch.zeros(n, 1), torch.zeros(n)), torch.zeros(n, 3),
                                        torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError, match="state must hold"):
        density.add_densification_stats(object(), torch.zeros(n, 3), torch.zeros(n, dtype=torch.int32))
    # max_grad
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="max_grad must be positive"):
            density.densify_and_prune(params, opt, st, **dict(kw, max_grad=bad))
    with pytest.raises(TypeError, match="max_grad must be a number"):
        density.densify_and_prune(params, opt, st, **dict(kw, max_grad=None))
    # group names
    short = {k: v for k, v in params.items() if k != "f_rest"}
    with pytest.raises(KeyError, match="params lacks the group 'f_rest'"):
        density.densify_and_prune(short, opt, st, **kw)
    opt2 = torch.optim.Adam([{"params": [p], "name": k} for k, p in short.items()], lr=1e-3)
    with pytest.raises(KeyError, match="optimizer has no group named 'f_rest'"):
        density.densify_and_prune(params, opt2, st, **kw)
    opt3 = torch.optim.Adam([{"params": [p]} for p in params.values()], lr=1e-3)
    with pytest.raises(ValueError, match="needs a \"name\""):
        density.densify_and_prune(params, opt3, st, **kw)
    with pytest.raises(ValueError, match="is not the parameter the optimizer holds"):
        density.densify_and_prune(dict(params, xyz=torch.nn.Parameter(params["xyz"].detach().clone())), opt, st, **kw)
    # mismatched N, wrong shapes
    with pytest.raises(ValueError, match="max_radii2D holds 15 rows"):
        density.densify_and_prune(params, opt, density.DensityState.zeros(n - 1, "cpu"), **kw)
    p_bad, o_bad = _model(n)
    p_bad["rotation"].data = torch.zeros(n, 3)
    with pytest.raises(ValueError, match=r"params\['rotation'\] must be \[N, 4\]"):
        density.densify_and_prune(p_bad, o_bad, st, **kw)
    p_bad, o_bad = _model(n)
    p_bad["opacity"].data = torch.zeros(n - 2, 1)
    with pytest.raises(ValueError, match=r"params\['opacity'\] holds 14 rows"):
        density.densify_and_prune(p_bad, o_bad, st, **kw)
    p_bad, o_bad = _model(n)
    p_bad["scaling"].data = torch.zeros(n, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"params\['scaling'\] must be torch.float32"):
        density.opacity_prune(p_bad, o_bad, st, 0.005)


def test_c_entry_points_refuse_bad_arguments(lib_built):
    """The C layer's own checks return an error code before any launch (no GPU is needed to see them)."""
    import ctypes as C
    from texgs import _lib
    lib = _lib.load()
    assert lib.texgs_density_stats(None, None, 4, None, None, None, None) != 0
    assert b"NULL" in lib.texgs_last_error()
    assert lib.texgs_density_stats(None, None, -1, None, None, None, None) != 0
    plan = _lib.DensityPlanStruct(None, None, None, None, 4, 0.0, 0.005, 0.01, 0.1, 1, 1)
    assert lib.texgs_density_plan(C.byref(plan), None, None, None, None, None) != 0
    plan = _lib.DensityPlanStruct(1, 1, 1, 1, 4, 0.0, 0.005, 0.01, 0.1, 1, 1)
    assert lib.texgs_density_plan(C.byref(plan), 1, 1, 1, 1, None) != 0
    assert b"max_grad must be positive" in lib.texgs_last_error()
    move = _lib.DensityMoveStruct()
    move.rows, move.n, move.n_kept, move.n_split, move.n_child = 25, 4, 4, 0, 0
    assert lib.texgs_density_move(C.byref(move), None) != 0
    assert b"rows must be" in lib.texgs_last_error()
    move.rows, move.n_kept = 1, 5
    assert lib.texgs_density_move(C.byref(move), None) != 0
    assert b"totals exceed n" in lib.texgs_last_error()
    move.n_kept, move.action, move.rank = 4, 1, 1
    move.row[0] = _lib.DensityRowStruct(1, 1, 4, _lib.DENSITY_ROW["xyz"])
    assert lib.texgs_density_move(C.byref(move), None) != 0
    assert b"XYZ row has width 3" in lib.texgs_last_error()
    assert lib.texgs_density_plan_temp_bytes(300001) >= 16 * 293


def test_header_exports_and_abi_version(lib_built):
    from texgs import _lib
    hdr = open(os.path.join(ROOT, "include", "texgs.h")).read()
    for name in ("texgs_density_stats", "texgs_density_plan_temp_bytes", "texgs_density_plan", "texgs_density_move"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.load(), name)
    m = re.search(r"#define\s+TEXGS_ABI_VERSION\s+(\d+)\b", hdr)
    assert _lib.load().texgs_abi_version() == _lib.ABI_VERSION == int(m.group(1))
    for k, v in dict(KEEP=_lib.DENSITY_KEEP, CLONE=_lib.DENSITY_CLONE, CLONE_KEPT=_lib.DENSITY_CLONE_KEPT, SPLIT=_lib.DENSITY_SPLIT,
                     CHILD=_lib.DENSITY_CHILD, MAX_ROWS=_lib.DENSITY_MAX_ROWS).items():
        assert re.search(r"#define\s+TEXGS_DENSITY_%s\s+%d\b" % (k, v), hdr), k
    for k, v in _lib.DENSITY_ROW.items():
        assert re.search(r"#define\s+TEXGS_DENSITY_ROW_%s\s+%d\b" % (k.upper(), v), hdr), k
    assert (R.KEEP, R.CLONE, R.CLONE_KEPT, R.SPLIT, R.CHILD) == (_lib.DENSITY_KEEP, _lib.DENSITY_CLONE, _lib.DENSITY_CLONE_KEPT,
                                                                 _lib.DENSITY_SPLIT, _lib.DENSITY_CHILD)


def test_struct_layouts_match_the_header(tmp_path):
    """The size and every field offset of the three new structs as a C compiler sees the header against the ctypes declarations (gcc, as
    tests/test_abi.py compiles its probe: a machine without it fails here, it does not skip)"""
    from texgs import _lib
    structs = {"TexGSDensityPlan": _lib.DensityPlanStruct, "TexGSDensityRow": _lib.DensityRowStruct, "TexGSDensityMove": _lib.DensityMoveStruct}
    consts = {"sizeof(((TexGSDensityMove*)0)->row) / sizeof(TexGSDensityRow)": _lib.DENSITY_MAX_ROWS, "TEXGS_DENSITY_MAX_ROWS": _lib.DENSITY_MAX_ROWS}
    assert abi_check.layout_mismatches("texgs.h", structs, consts, tmp_path) == []
