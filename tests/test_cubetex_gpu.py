"""-m gpu: seamless cubemap sampling (texgs.cubetex, csrc/cubetex.hip) against its float64 statement (tests/cubetex_ref.py).

The forward bound is derived, not tuned: from the direction to (col, row) the kernel makes a handful of fp32 roundings on values
<= 1 that are then scaled by R/2, so (col, row) is off by at most 8 * 2^-23 * R/2 texel, and a bilinear fetch moves by at most
(max tex - min tex) per texel; the weights and the four products add a few roundings of the values themselves:
    tol = 8 * 2^-23 * (R/2) * (max tex - min tex) + 8 * 2^-23 * max|tex|.
Every test prints the largest error it measured next to its bound.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubetex_ref as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = 8.0 * 2.0 ** -23


def cubetex():
    from texgs import cubetex as m
    return m


def tol_forward(R, tex):
    tex = tex.double()
    return U8 * (R / 2.0) * float(tex.max() - tex.min()) + U8 * float(tex.abs().max())


def face_points(face, col, row, R):
    """float64 directions (not normalised) of the points (col, row), in texels, of `face`"""
    s = (col + 0.5) * (2.0 / R) - 1.0
    t = (row + 0.5) * (2.0 / R) - 1.0
    return O.cube_to_dir(face, s, t)


def leaf(x):
    return x.detach().to(DEV).clone().requires_grad_()


def report(name, err, bound):
    print(f"{name}: max error {err:.3e}, bound {bound:.3e}")


# ---- seams ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [4, 5])
def test_seams_exhaustively(R):
    """Every texel holds its own index, so a tap on a wrong face, edge or position along the edge changes the result by its weight
    (at least 1/64 on this grid) times an index difference of at least 1: more than 30 times the bound, and most such taps miss by
    far more.  Queries: a 4x oversampled grid (offset by 1/8 texel, so none sits on a texel boundary) over the bands within 1.5
    texels of every edge of every face."""
    tex = torch.arange(6 * R * R, dtype=torch.float32).reshape(6, R, R, 1)
    p = torch.arange(4 * R, dtype=torch.float64) * 0.25 - 0.5 + 0.125          # in (-0.5, R - 0.5)
    col, row = torch.meshgrid(p, p, indexing="xy")
    near = (col < 1.0) | (col > R - 2.0) | (row < 1.0) | (row > R - 2.0)
    col, row = col[near], row[near]
    dirs, faces = [], []
    for f in range(6):
        face = torch.full(col.shape, f)
        dirs.append(face_points(face, col, row, R) * (0.5 + f))                # any length
        faces.append(face)
    dirs = torch.cat(dirs).float()
    faces = torch.cat(faces)
    want, kinds = O.sample(tex, dirs, return_taps=True)
    # the input really covers all 24 directed edges and, from each of its three faces, all 8 corners
    assert torch.equal(O.address(dirs.double(), R)[0], faces)
    edges = {(int(f), int(k) - 1) for f, ks in zip(faces, kinds) for k in ks if k > 0}
    assert len(edges) == 24
    corner_taps = {(int(f), int((ks == -1).nonzero()[0])) for f, ks in zip(faces, kinds) if (ks == -1).any()}
    assert len(corner_taps) == 24
    got = cubetex().cube_sample(tex.to(DEV), dirs.to(DEV)).cpu().double()
    err, bound = float((got - want).abs().max()), tol_forward(R, tex)
    report(f"seams R={R} N={dirs.shape[0]}", err, bound)
    assert err <= bound


# ---- random interior and edges -----------------------------------------------------------------------------------------------------

def random_dirs(n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return (d * (0.1 + 9.9 * torch.rand(n, 1, generator=g, dtype=torch.float64))).float()


@pytest.mark.parametrize("N", [1, 63, 1000])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_random_directions(C, N):
    R = 16
    g = torch.Generator().manual_seed(100 * C + N)
    tex = torch.randn(6, R, R, C, generator=g)
    dirs = random_dirs(N, 7 * C + N)
    ct = cubetex()
    got = ct.cube_sample(tex.to(DEV), dirs.to(DEV)).cpu().double()
    assert tuple(got.shape) == (N, C)
    err, bound = float((got - O.sample(tex, dirs)).abs().max()), tol_forward(R, tex)
    report(f"linear R={R} C={C} N={N}", err, bound)
    assert err <= bound
    # nearest is exact away from the decision boundaries: the texel boundary (fp32 col is off by ~1e-5 texel at most) and the tie
    # of the two largest components
    _, col, row = O.address(dirs.double(), R)
    a = dirs.double().abs().sort(dim=1, descending=True)[0]
    frac = lambda v: (v + 0.5 - torch.round(v + 0.5)).abs()        # noqa: E731
    excluded = (frac(col) < 1e-3) | (frac(row) < 1e-3) | ((a[:, 0] - a[:, 1]) < 1e-4 * a[:, 0])
    assert int(excluded.sum()) <= 0.02 * N
    got = ct.cube_sample(tex.to(DEV), dirs.to(DEV), "nearest").cpu()
    want = O.sample(tex, dirs, "nearest").float()
    assert torch.equal(got[~excluded], want[~excluded])


def test_nearest_gradient_reaches_the_texture_only():
    R, C, N = 16, 3, 1000
    g = torch.Generator().manual_seed(5)
    tex = torch.randn(6, R, R, C, generator=g)
    dirs = random_dirs(N, 6)
    _, col, row = O.address(dirs.double(), R)
    keep = ((col + 0.5 - torch.round(col + 0.5)).abs() > 1e-3) & ((row + 0.5 - torch.round(row + 0.5)).abs() > 1e-3)
    dirs = dirs[keep]
    go = torch.rand(dirs.shape[0], C, generator=g) - 0.5
    t = leaf(tex)
    d = leaf(dirs)
    cubetex().cube_sample(t, d, "nearest").backward(go.to(DEV))
    assert d.grad is None
    f, x, y = O.nearest_texel(dirs.double(), R)
    want = torch.zeros(6 * R * R, C, dtype=torch.float64).index_add_(0, (f * R + y) * R + x, go.double()).reshape(6, R, R, C)
    touching = torch.zeros(6 * R * R, C, dtype=torch.float64).index_add_(0, (f * R + y) * R + x, go.double().abs()).reshape(6, R, R, C)
    assert bool(((t.grad.cpu().double() - want).abs() <= 2.0 ** -20 * touching).all())


# ---- tap transform ----------------------------------------------------------------------------------------------------------------

def test_tap_transform_is_applied_per_tap():
    R, C, N = 8, 3, 1000
    g = torch.Generator().manual_seed(11)
    tex = torch.rand(6, R, R, C, generator=g) * 6.0 - 3.0          # 0.282 * 3 + 0.5 = 1.35 and -0.35: both clamps fire
    assert float(O.sh02rgb(tex.double()).max()) == 1.0 and float(O.sh02rgb(tex.double()).min()) == 0.0
    dirs = random_dirs(N, 12)
    ct = cubetex()
    got = ct._forward(tex.to(DEV), dirs.to(DEV), "linear", True).cpu().double()
    want = O.sample(tex, dirs, tap_map=True)
    assert torch.equal(want, O.sample(O.sh02rgb(tex.double()), dirs))
    err, bound = float((got - want).abs().max()), tol_forward(R, O.sh02rgb(tex.double()))
    report(f"tap transform R={R} C={C} N={N}", err, bound)
    assert err <= bound
    after = O.sh02rgb(ct.cube_sample(tex.to(DEV), dirs.to(DEV)).cpu().double())          # clamping after the filter is another function
    assert float((got - after).abs().max()) > 0.05


# ---- fused lat-long ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", [(8, 16), (6, 10)])
def test_fused_latlong(res):
    R, C = 8, 3
    g = torch.Generator().manual_seed(res[0])
    tex = torch.rand(6, R, R, C, generator=g) * 6.0 - 3.0
    ct = cubetex()
    t = tex.to(DEV)
    dirs64 = O.latlong_dirs(res).reshape(-1, 3)
    dirs32 = ct.latlong_dirs(res, DEV)
    for name, got, composed, want, rng in (
            ("cubemap_to_latlong", ct.cubemap_to_latlong(t, res), ct.cube_sample(t, dirs32), O.sample(tex, dirs64), tex),
            ("sphere_map", ct.sphere_map(t, res), ct.cube_sample(O.sh02rgb(t), dirs32), O.sample(tex, dirs64, tap_map=True),
             O.sh02rgb(tex.double()))):
        assert tuple(got.shape) == res + (C,) and tuple(composed.shape) == res + (C,)
        bound = tol_forward(R, rng)
        want = want.reshape(res + (C,))
        e1 = float((got.cpu().double() - want).abs().max())
        e2 = float((composed.cpu().double() - want).abs().max())
        e3 = float((got - composed).abs().max())
        report(f"{name} {res} fused against the statement", e1, bound)
        report(f"{name} {res} composition against the statement", e2, bound)
        report(f"{name} {res} fused against the composition", e3, bound)
        assert e1 <= bound and e2 <= bound and e3 <= bound


# ---- degenerate rows --------------------------------------------------------------------------------------------------------------

def test_degenerate_rows():
    R, C, N = 8, 3, 130
    g = torch.Generator().manual_seed(21)
    tex = torch.randn(6, R, R, C, generator=g)
    dirs = random_dirs(N, 22)
    bad = {0: [0.0, 0.0, 0.0], 5: [float("nan"), 1.0, 0.0], 63: [float("inf"), 0.0, 0.0], 64: [1.0, float("-inf"), 2.0],
           65: [-0.0, 0.0, -0.0], 100: [1.0, 2.0, float("nan")], 129: [float("inf"), float("inf"), float("nan")]}
    for i, v in bad.items():
        dirs[i] = torch.tensor(v)
    is_bad = torch.zeros(N, dtype=torch.bool)
    is_bad[list(bad)] = True
    assert torch.equal(O.degenerate(dirs), is_bad)
    go = torch.rand(N, C, generator=g) - 0.5
    ct = cubetex()

    def run(d, g_out):
        t = leaf(tex)
        dd = leaf(d)
        out = ct.cube_sample(t, dd)
        out.backward(g_out.to(DEV))
        return out.detach().cpu(), t.grad.cpu(), dd.grad.cpu()
    out, d_tex, d_dirs = run(dirs, go)
    out_good, d_tex_good, d_dirs_good = run(dirs[~is_bad], go[~is_bad])
    assert torch.equal(out[is_bad], torch.zeros(len(bad), C))
    assert torch.equal(d_dirs[is_bad], torch.zeros(len(bad), 3))
    assert torch.equal(out[~is_bad], out_good)                       # their neighbours are unaffected
    assert torch.equal(d_dirs[~is_bad], d_dirs_good)
    assert bool(torch.isfinite(d_tex).all())
    assert torch.allclose(d_tex, d_tex_good, rtol=0, atol=1e-5)     # (atomics: the order of the sum differs between the runs)
    assert float((out[~is_bad].double() - O.sample(tex, dirs[~is_bad])).abs().max()) <= tol_forward(R, tex)


# ---- gradients --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grad_scene():
    """R = 5, C = 3, N = 1000 unit directions: 904 random ones, 72 in the outer half-texel band of a face (3 for each of the 24
    directed edges; their footprint has two taps across the edge) and 24 in the outer half-texel square at a face's corner (each of
    the 8 cube corners from its 3 faces; their footprint has a tap across each edge and the dropped one).  g is uniform in [-1, 1].
    The statement and its autograd are computed once, here."""
    R, C = 5, 3
    g = torch.Generator().manual_seed(31)
    tex = torch.randn(6, R, R, C, generator=g)
    parts = [torch.randn(904, 3, generator=g, dtype=torch.float64)]
    inner = torch.tensor([1.3, 2.4, 2.7], dtype=torch.float64)            # along the edge, away from its ends
    for f in range(6):
        face = torch.full((3,), f)
        for out_of_face in (-0.25, R - 0.75):
            parts.append(face_points(face, torch.full((3,), out_of_face, dtype=torch.float64), inner, R))
            parts.append(face_points(face, inner, torch.full((3,), out_of_face, dtype=torch.float64), R))
        for cx in (-0.27, R - 0.73):
            for cy in (-0.23, R - 0.77):
                parts.append(face_points(face[:1], torch.tensor([cx], dtype=torch.float64), torch.tensor([cy], dtype=torch.float64), R))
    dirs = torch.cat(parts)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).float()
    assert dirs.shape[0] == 1000
    go = torch.rand(1000, C, generator=g) * 2.0 - 1.0
    t64 = tex.double().requires_grad_()
    d64 = dirs.double().requires_grad_()
    out, touching, kinds = O.sample(t64, d64, touching_abs=go, return_taps=True)
    out.backward(go.double())
    return dict(R=R, C=C, tex=tex, dirs=dirs, go=go, out=out.detach(), d_tex=t64.grad, d_dirs=d64.grad, touching=touching, kinds=kinds)


@pytest.fixture(scope="module")
def grad_gpu(grad_scene):
    s = grad_scene
    t = leaf(s["tex"])
    d = leaf(s["dirs"])
    out = cubetex().cube_sample(t, d)
    out.backward(s["go"].to(DEV))
    return out.detach().cpu().double(), t.grad.cpu().double(), d.grad.cpu().double()


def test_texture_gradient(grad_scene, grad_gpu):
    """A tap weight is a product of two of {fx, 1 - fx, fy, 1 - fy}: fx is off by the error of col, 8 * 2^-23 * R/2, and the
    product, the renormalisation and the multiplication by g add a few roundings: tol_w = 8 * 2^-23 * R/2 + 2^-20 per unit of |g|,
    summed over the queries that touch the texel (the sum of the fp32 atomics themselves is covered by the 2^-20)."""
    s, (_, d_tex, _) = grad_scene, grad_gpu
    tol_w = U8 * s["R"] / 2.0 + 2.0 ** -20
    diff = (d_tex - s["d_tex"]).abs()
    bound = tol_w * s["touching"]
    worst = float((diff / bound.clamp_min(1e-30)).max())
    print(f"texture gradient: max error {float(diff.max()):.3e}, max error / bound {worst:.3f} (tol_w = {tol_w:.3e})")
    assert bool((diff <= bound).all())
    tot, want = d_tex.sum(dim=(0, 1, 2)), s["go"].double().sum(0)
    print("sum of d_texture per channel:", tot.tolist(), "sum of g:", want.tolist())
    assert bool(((tot - want).abs() <= 1e-5 * want.abs()).all())          # the weights sum to one, at the corners too


def test_direction_gradient(grad_scene, grad_gpu):
    """Checked where the gradient is continuous: >= 0.02 texel from every integer col and row (there the footprint changes) and
    with the dominant axis leading by >= 1e-3 relative (there the face changes).  d out / d col is a difference of texels weighted
    by fy, so it carries the forward's error per texel; d col / d dir is (R/2)/ma <= (R/2)/ma_min with ma_min = 1/sqrt(3) on unit
    directions, and there are two such terms: (R/ma_min) * tol_forward + 1e-6 |ref|, for |g| <= 1 per channel."""
    s, (_, _, d_dirs) = grad_scene, grad_gpu
    R = s["R"]
    d = s["dirs"].double()
    _, col, row = O.address(d, R)
    a = d.abs().sort(dim=1, descending=True)[0]
    keep = ((col - torch.round(col)).abs() >= 0.02) & ((row - torch.round(row)).abs() >= 0.02) & ((a[:, 0] - a[:, 1]) >= 1e-3 * a[:, 0])
    assert int(keep.sum()) >= 0.85 * d.shape[0]
    kinds = s["kinds"][keep]
    corner = (kinds == -1).any(1)
    edge = (kinds > 0).any(1) & ~corner
    print(f"direction gradient: {int(keep.sum())} of {d.shape[0]} queries checked, {int(edge.sum())} with a footprint across an edge, "
          f"{int(corner.sum())} in a corner footprint")
    assert int(edge.sum()) >= 50 and int(corner.sum()) >= 8
    ref = s["d_dirs"][keep]
    diff = (d_dirs[keep] - ref).abs()
    bound = (R * 3.0 ** 0.5) * tol_forward(R, s["tex"]) + 1e-6 * ref.abs()
    print(f"direction gradient: max error {float(diff.max()):.3e} (edge {float(diff[edge].max()):.3e}, corner "
          f"{float(diff[corner].max()):.3e}), max error / bound {float((diff / bound).max()):.3f}, max |ref| {float(ref.abs().max()):.3e}")
    assert bool((diff <= bound).all())


def test_gradient_scene_forward(grad_scene, grad_gpu):
    s, (out, _, _) = grad_scene, grad_gpu
    err, bound = float((out - s["out"]).abs().max()), tol_forward(s["R"], s["tex"])
    report("gradient scene forward R=5 C=3 N=1000", err, bound)
    assert err <= bound


# ---- the nvdiffrast drop-in and the chessboard --------------------------------------------------------------------------------------

def test_nvdiffrast_drop_in():
    import nvdiffrast.torch as dr
    R, C, N = 8, 3, 500
    g = torch.Generator().manual_seed(41)
    tex = torch.randn(6, R, R, C, generator=g).to(DEV)
    dirs = random_dirs(N, 42).to(DEV)
    ct = cubetex()
    got = dr.texture(tex[None], dirs[None, None], boundary_mode="cube")
    assert tuple(got.shape) == (1, 1, N, C)
    assert torch.equal(got[0, 0], ct.cube_sample(tex, dirs))
    assert torch.equal(dr.texture(tex[None], dirs[None, None], filter_mode="linear", boundary_mode="cube"), got)
    assert torch.equal(dr.texture(tex[None], dirs[None, None], filter_mode="nearest", boundary_mode="cube")[0, 0],
                       ct.cube_sample(tex, dirs, "nearest"))
    two = torch.stack([tex, -tex])
    d2 = torch.stack([dirs, dirs.flip(0)])[:, None]
    got2 = dr.texture(two, d2, boundary_mode="cube")
    assert torch.equal(got2[1, 0], ct.cube_sample(-tex, dirs.flip(0)))
    assert torch.equal(dr.texture(tex[None], d2, boundary_mode="cube")[1, 0], ct.cube_sample(tex, dirs.flip(0)))


def test_chessboard_texture():
    dirs = random_dirs(500, 43)
    got = cubetex().chessboard_texture(dirs.to(DEV)).cpu().double()
    board = O.chessboard(6)
    assert tuple(board.shape) == (6, 96, 96, 3) and tuple(got.shape) == (500, 3)
    err, bound = float((got - O.sample(board, dirs)).abs().max()), tol_forward(96, board)
    report("chessboard R=96 N=500", err, bound)
    assert err <= bound
    boards = dict(cubetex()._BOARDS)
    cubetex().chessboard_texture(dirs[:3].to(DEV))
    assert len(boards) >= 1 and all(cubetex()._BOARDS[k] is v for k, v in boards.items()) and len(cubetex()._BOARDS) == len(boards)
