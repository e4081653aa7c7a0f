"""K1 / K8 alone, on the CPU: the scenes of preprocess_ref.py hold their guards, the moment convention of csrc/common.h (M_* -> R_*)
agrees with the blend formulas to 1e-10, and the fp32 C oracle (texgs_ref_preprocess, texgs_ref_preprocess_bwd) -- the yardstick the
HIP kernels are held to in test_preprocess_gpu.py -- stays within 1e-4 of float64 on every visible row of the well-conditioned regimes
(2e-3 on "shipped shape"), no row excluded.  The measured figures go to profiles/preprocess_parity.json under "c_oracle_vs_f64"."""
import numpy as np
import pytest
import torch

import helpers as Hh
import preprocess_ref as PR
from oracle import texgs_ref as CR

CASES = pytest.mark.parametrize("regime,flavour", PR.ALL_CASES, ids=[f"{r}-{f}" for r, f in PR.ALL_CASES])
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _record_figures():
    yield
    PR.store_parity("c_oracle_vs_f64", _FIGURES)


def _note(case, figures):
    _FIGURES.setdefault(case.name, {}).setdefault(case.flavour, {}).update(figures)
    Hh.report(f"preprocess/c_oracle_vs_f64/{case.name}/{case.flavour}", **figures)


def c_oracle(case):
    run = CR.RefRun(case.scene, case.settings())
    run.forward()
    return run


def c_backward(run, case, M32):
    g = run._preprocess_bwd(PR.cotangent_f32(M32.numpy(), run.rec[:case.N]).astype(np.float64))
    return {("cov3D" if n == "cov3D" else n): torch.tensor(v) for n, v in g.items() if v is not None}


@CASES
def test_scene_guards_and_visibility(regime, flavour):
    """The builder's own assertions (floor on the count, every decision >= 1e-4 clear of its threshold) hold, and fp32 and float64
    then agree on every visibility decision."""
    p = PR.prepared(regime, flavour)
    run = c_oracle(p.case)
    assert torch.equal(torch.tensor(run.radii[:p.case.N] > 0), p.visible)
    assert np.array_equal(run.radii[:p.case.N], p.pre["radius"].numpy().astype(np.int32))
    assert p.case.N <= 1500 and (p.case.cam.image_width, p.case.cam.image_height) == (136, 88)


@CASES
def test_moment_convention(regime, flavour):
    """autograd of L_pairs (the blend formulas on the pairs) == autograd of <cotangent_from_moments(M), record64>, M unrounded, every
    row, 1e-10 relative: the M_* -> R_* map of common.h."""
    p = PR.prepared(regime, flavour)
    a = PR.grads_of(p.case, lambda pre: PR.pair_loss(pre, p.pairs, p.case.textured))
    b = PR.reference_grads(p.case, p.M)
    for n in PR.INPUTS[flavour]:
        assert float(a[n].abs().max()) > 0 or n in ("uvs",) or p.case.sh_degree == 0, n
        assert PR.row_error(b[n], a[n]) <= 1e-10, (n, PR.row_error(b[n], a[n]))
        assert float(a[n][~p.visible].abs().max() if bool((~p.visible).any()) else 0.0) == 0.0


@CASES
def test_c_oracle_records(regime, flavour):
    """RefRun.rec against record64, field by field, every visible row"""
    p = PR.prepared(regime, flavour)
    run = c_oracle(p.case)
    rec = torch.tensor(run.rec[:p.case.N])
    figs = {f"rec_{k}": PR.row_error(rec[:, a:b], p.rec[:, a:b], p.visible) for k, (a, b) in PR.FIELDS.items()}
    _note(p.case, figs)
    for k, v in figs.items():
        assert v <= p.case.bar, (k, v)
    assert not rec[~p.visible].any()


@CASES
def test_c_oracle_backward(regime, flavour):
    """float32 cotangent from the f32 moments through texgs_ref_preprocess_bwd against float64 autograd, every visible row; culled
    rows exactly zero"""
    p = PR.prepared(regime, flavour)
    got = c_backward(c_oracle(p.case), p.case, p.M32)
    figs = {n: PR.row_error(got[n], p.ref[n], p.visible) for n in PR.INPUTS[flavour]}
    _note(p.case, figs)
    for n, v in figs.items():
        assert v <= p.case.bar, (n, v)
        assert not got[n][~p.visible].any(), n
    assert not got["means2D"][:, 2].any()


def test_degenerate_plane_sends_nothing_from_the_uv_cotangents():
    """|sdot| <= 0.05 |t|: G = g = 0 in float64 and in the C oracle, and other values in the G / g cotangent slots change nothing in
    those rows (bit for bit); the rows beside them do move."""
    p = PR.prepared("degenerate_plane")
    deg, reg = p.case.masks["degenerate"], p.case.masks["regular"]
    run = c_oracle(p.case)
    assert not p.rec[deg][:, PR.R_G2:PR.R_PHI].any() and not run.rec[:p.case.N][deg.numpy()][:, PR.R_G2:PR.R_PHI].any()
    assert bool(p.rec[reg][:, PR.R_G2:PR.R_PHI].abs().max(1).values.min() > 0)
    a, b = c_backward(run, p.case, p.M32), c_backward(run, p.case, PR.other_uv_cotangents(p.M32))
    for n in PR.INPUTS["textured"]:
        assert torch.equal(a[n][deg], b[n][deg]), n
    assert not torch.equal(a["means3D"][reg], b["means3D"][reg])


@pytest.mark.parametrize("regime", ["general", "clamp", "camera"])
def test_cov3d_gradient_layout(regime):
    """cov3D_precomp: dL/dcov3D in the lineage layout -- float64 autograd with respect to the six stored entries gives the off-diagonal
    ones both symmetric halves --, and nothing flows through the eigenvector normal: other dL/dnormal sums change no output."""
    p = PR.prepared(regime, "cov")
    run = c_oracle(p.case)
    a = c_backward(run, p.case, p.M32)
    full = PR.full_matrix_cov_gradient(p.case, p.M32.to(PR.F64))          # dL/dSigma as a full symmetric 3x3 matrix
    lineage = torch.stack([full[:, 0, 0], full[:, 0, 1] + full[:, 1, 0], full[:, 0, 2] + full[:, 2, 0], full[:, 1, 1],
                           full[:, 1, 2] + full[:, 2, 1], full[:, 2, 2]], 1)
    assert PR.row_error(lineage, p.ref["cov3D"]) <= 1e-10
    assert PR.row_error(a["cov3D"], lineage, p.visible) <= p.case.bar
    M2 = p.M32.clone()
    M2[:, PR.M_N:PR.M_N + 3] = 0.0
    b = c_backward(run, p.case, M2)
    for n in PR.INPUTS["cov"]:
        assert torch.equal(a[n], b[n]), n
    ref2 = PR.reference_grads(p.case, M2.to(PR.F64))
    for n in PR.INPUTS["cov"]:
        assert torch.equal(ref2[n], p.ref[n]), n
