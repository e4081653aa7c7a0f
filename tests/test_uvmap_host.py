"""-m "not gpu": the UV-map stage's host side -- the hash-grid statement (level table, dense / hashed corners, the x = 1 wrap, its
input gradient), the tiny-cuda-nn state loader of InvUVNet, loud failure on CPU tensors, the C layout of the new struct."""
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import hashgrid_ref as R  # noqa: E402


def test_shipped_level_table():
    lv, n = R.levels(**R.SHIPPED)
    assert [r for _, r, _, _, _ in lv] == [16, 24, 34, 49, 71, 102, 147, 213]
    assert [sz for _, _, sz, _, _ in lv] == [4096] * 8
    assert [h for *_, h in lv] == [False] + [True] * 7           # 16^3 = 4096 fits the table exactly: level 0 is dense
    assert n == 131072


def test_library_level_table_matches_the_statement(lib_built):
    from texgs import uvmap
    got = uvmap.hashgrid_levels()
    lv, n = R.levels(**R.SHIPPED)
    assert got["n_params"] == n
    assert got["scale"] == [s for s, *_ in lv]                    # bit-equal fp32 scales
    assert got["res"] == [r for _, r, *_ in lv]
    assert got["size"] == [sz for _, _, sz, _, _ in lv]
    assert got["offset"] == [o for _, _, _, o, _ in lv]
    with pytest.raises(ValueError, match="n_features must be 4"):
        uvmap.hashgrid_levels(n_features=2)
    with pytest.raises(ValueError, match="n_levels"):
        uvmap.hashgrid_levels(n_levels=17)


@pytest.mark.parametrize("name", sorted(R.GRIDS))
def test_library_level_table_matches_the_statement_off_the_shipped_grid(lib_built, name):
    """Every grid of hashgrid_ref.GRIDS: the library's host arithmetic (exp2f / log2f in fp32) and the statement's agree field by
    field, bit-equal scales included, and both give the row counts the grid was chosen for.  small_dense has scales that are
    integers mathematically (3, 5, 8): an exp2f one ulp above would change res and every offset after it."""
    from texgs import uvmap
    grid = R.GRIDS[name]
    got = uvmap.hashgrid_levels(**grid)
    lv, n = R.levels(**dict(R.SHIPPED, **grid))
    assert len(lv) == grid["n_levels"] == len(got["scale"])
    assert got["n_params"] == n == 4 * sum(R.GRID_SIZES[name])
    assert got["scale"] == [s for s, *_ in lv]                    # bit-equal fp32 scales
    assert got["res"] == [r for _, r, *_ in lv]
    assert got["size"] == [sz for _, _, sz, _, _ in lv] == R.GRID_SIZES[name]
    assert got["offset"] == [o for _, _, _, o, _ in lv]
    assert all(sz % 8 == 0 for sz in got["size"])
    if name == "small_dense":
        assert got["scale"][:5] == [3.0, 5.0, 8.0, 12.5, 19.25] and abs(got["scale"][5] - 29.375) < 1e-5
        assert got["res"] == [4, 6, 9, 14, 21, 31]
    if name == "mixed":
        assert [h for *_, h in lv] == [False, False, True, True, True]


def test_rounding_bar():
    assert R.rounding_bar(1.0) == 2.0 ** -17 + 8 * 2.0 ** -24                  # the shipped grid: pos < 256
    assert R.rounding_bar(1.15, **R.GRIDS["mixed"]) == 2.0 ** -18 + 8 * 2.0 ** -24     # 69.14 * 1.15 + 0.5 = 80.0: [64, 128)
    assert R.rounding_bar(1.15, **R.GRIDS["small_dense"]) == 2.0 ** -19 + 8 * 2.0 ** -24       # 29.37 * 1.15 + 0.5 = 34.3
    assert R.rounding_bar(1.15, **R.GRIDS["L1"]) == 2.0 ** -20 + 8 * 2.0 ** -24        # 15 * 1.15 + 0.5 = 17.75


def test_touch_sums_by_hand():
    # one point in the middle of cell (1, 2, 3) of the 16^3 level: its 8 corners are 8 distinct rows, each touched once
    x = torch.tensor([[1.0 / 15, 2.0 / 15, 3.0 / 15]], dtype=torch.float64)
    de = torch.tensor([[1.0, -2.0, 3.0, -4.0]])
    T, cnt = R.touch_sums(x, de, **R.GRIDS["L1"])
    rows = sorted((1 + (c & 1)) + 16 * (2 + ((c >> 1) & 1)) + 256 * (3 + (c >> 2)) for c in range(8))
    assert sorted(set((cnt.nonzero()[:, 0] // 4).tolist())) == rows
    assert int(cnt.sum()) == 8 * 4 and int(cnt.max()) == 1
    assert T.reshape(-1, 4)[rows[0]].tolist() == [1.0, 2.0, 3.0, 4.0] and float(T.sum()) == 80.0


def test_level0_is_dense():
    g = torch.randint(0, 16, (200, 3))
    idx = R.corner_index(g[:, 0], g[:, 1], g[:, 2], 16, 4096, False)
    assert torch.equal(idx, g[:, 0] + 16 * g[:, 1] + 256 * g[:, 2])


def test_hashed_corner_by_hand():
    # level 1: res 24, 24^3 = 13824 > 4096 -> hashed.  p = (3, 5, 7):
    # 5 * 2654435761 = 13272178805 = 387276917 mod 2^32;  7 * 805459861 = 5638219027 = 1343251731 mod 2^32
    # low 12 bits: 3, 117, 1299 -> 3 ^ 117 ^ 1299 = 1381
    assert int(R.corner_index(3, 5, 7, 24, 4096, True)) == 1381


def test_x_equal_one_wraps():
    # level 0 at x = 1: pos = 15 + 0.5, g = 15, the c = 1 corner is p = 16 = res: dense index 16 + 16*16 + 256*16 = 4368 -> % 4096 = 272
    assert int(R.corner_index(16, 16, 16, 16, 4096, False)) == 272
    params = torch.randn(131072, dtype=torch.float64)
    x = torch.ones(1, 3, dtype=torch.float64)
    enc = R.encode(x, params)
    tab = params.reshape(-1, 4)
    rows = [R.corner_index(15 + (c & 1), 15 + ((c >> 1) & 1), 15 + (c >> 2), 16, 4096, False) for c in range(8)]
    assert torch.allclose(enc[0, :4], sum(tab[int(r)] for r in rows) / 8)
    assert torch.isfinite(enc).all()


def test_statement_input_gradient_against_finite_differences():
    g = torch.Generator().manual_seed(4)
    params = torch.randn(131072, generator=g, dtype=torch.float64)
    x = torch.rand(64, 3, generator=g, dtype=torch.float64) * 0.9 + 0.05
    keep = R.face_distance(x) > 1e-4                               # central differences of h = 1e-7 cell-units never cross a face
    x = x[keep].clone().requires_grad_(True)
    w = torch.randn(x.shape[0], 32, generator=g, dtype=torch.float64)
    (R.encode(x, params) * w).sum().backward()
    h = 1e-9                                                       # pos moves by at most 213 * 1e-9 = 2e-7 cells
    fd = torch.zeros_like(x)
    for d in range(3):
        e = torch.zeros_like(x)
        e[:, d] = h
        with torch.no_grad():
            fd[:, d] = ((R.encode(x + e, params) - R.encode(x - e, params)) * w).sum(1) / (2 * h)
    # the encoding is trilinear inside a cell: central differences are exact up to float64 cancellation, ~1e-16 * |enc| / h
    assert torch.allclose(x.grad, fd, rtol=1e-5, atol=1e-4), float((x.grad - fd).abs().max())


def _tcnn_state(dtype, g):
    return {"pre_mlp.0.params": torch.randn(131072, generator=g).to(dtype),
            "pre_mlp.1.params": (torch.randn(32 * 128 + 128 * 128, generator=g) * 0.1).to(dtype),
            "mlp.params": (torch.randn(2 * 128 * 128 + 16 * 128, generator=g) * 0.1).to(dtype)}


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_tcnn_state_loader(lib_built, dtype):
    from texgs import uvmap
    from texgs.uvnet import unpack_tcnn_params
    net = uvmap.InvUVNet()
    st = _tcnn_state(dtype, torch.Generator().manual_seed(1))
    with pytest.warns(RuntimeWarning, match="UNPINNED"):
        net.load_reference_state(st)
    assert net.tcnn_layout_unpinned
    assert net.encoding.params.dtype == torch.float32
    assert torch.equal(net.encoding.params.detach(), st["pre_mlp.0.params"].float())
    layers = unpack_tcnn_params(st["pre_mlp.1.params"], 32, 128, 1) + unpack_tcnn_params(st["mlp.params"], 128, 3, 2)
    for w, (ref, b) in zip(net._weights(), layers):
        assert b is None
        assert w.dtype == torch.float32 and torch.equal(w.detach(), ref)
    assert [tuple(w.shape) for w in net._weights()] == [(128, 32), (128, 128), (128, 128), (128, 128), (3, 128)]
    # its own state_dict round-trips and clears the flag
    other = uvmap.InvUVNet().load_reference_state(net.state_dict())
    assert not other.tcnn_layout_unpinned
    assert torch.equal(other.encoding.params, net.encoding.params)


def test_stage3_checkpoint_inv_uv_net(lib_built):
    from texgs import texture_io, uvmap
    from texgs.uvnet import unpack_tcnn_params
    st = texture_io.load_checkpoint(os.path.join(ROOT, "tests", "golden", "ckpt_stage3.pth"))
    inv = st.net_state[1]
    assert sorted(inv) == ["mlp.params", "pre_mlp.0.params", "pre_mlp.1.params"]
    pre = unpack_tcnn_params(inv["pre_mlp.1.params"], 32, 128, 1)
    mlp = unpack_tcnn_params(inv["mlp.params"], 128, 3, 2)
    assert [tuple(w.shape) for w, _ in pre + mlp] == [(128, 32), (128, 128), (128, 128), (128, 128), (3, 128)]
    assert all(b is None for _, b in pre + mlp)
    # the fixture's encoding is a 4096-value stand-in, not a shipped grid: refused with the count it needs
    with pytest.raises(ValueError, match="expected 131072"):
        uvmap.InvUVNet().load_reference_state(inv)


def test_reference_state_of_another_grid_is_refused(lib_built):
    """The table of a tiny-cuda-nn state is sized by its grid: a net built for one grid refuses the table of another, either way
    round, with the count it needs, and keeps its own parameters."""
    from texgs import uvmap
    g = torch.Generator().manual_seed(2)
    mixed = uvmap.InvUVNet(grid=R.GRIDS["mixed"])
    assert mixed.encoding.n_params == 268288 and mixed.encoding.n_output_dims == 20
    before = mixed.encoding.params.detach().clone()
    with pytest.raises(ValueError, match="expected 268288"):
        mixed.load_reference_state(_tcnn_state(torch.float32, g))                  # the shipped grid's 131072-value table
    assert torch.equal(mixed.encoding.params.detach(), before) and not mixed.tcnn_layout_unpinned
    st = _tcnn_state(torch.float32, g)
    st["pre_mlp.0.params"] = torch.randn(268288, generator=g)
    with pytest.raises(ValueError, match="expected 131072"):
        uvmap.InvUVNet().load_reference_state(st)


def test_wrong_sizes_raise_before_any_launch(lib_built):
    """The C ABI takes bare pointers: a table of the wrong size, a point array that is not [N, 3] or point sets on different
    devices must be refused by the Python layer (ValueError) before a kernel could index past them -- on any device."""
    from texgs import uvmap
    with pytest.raises(ValueError, match="expected a flat tensor of 131072"):
        uvmap.hashgrid_encode(torch.rand(4, 3), torch.zeros(4096, requires_grad=True))      # the stage-3 fixture's stand-in size
    with pytest.raises(ValueError, match=r"x must be \[N, 3\]"):
        uvmap.InvUVNet()(torch.rand(4, 2), torch.zeros(128))
    with pytest.raises(ValueError, match=r"x must be \[N, 3\]"):
        uvmap.HashGridEncoding()(torch.rand(4, 3, 1))
    with pytest.raises(ValueError, match="expected a flat tensor"):
        uvmap.hashgrid_encode(torch.rand(4, 3), torch.zeros(2, 65536))
    with pytest.raises(ValueError, match="expected a flat tensor of 8192"):
        uvmap.hashgrid_encode(torch.rand(4, 3), torch.zeros(131072), grid=dict(n_levels=2, log2_hashmap_size=10))
    with pytest.raises(ValueError, match=r"\[P, 3\] and \[Q, 3\]"):
        uvmap.nearest_neighbours(torch.rand(5, 2), torch.rand(7, 3))
    with pytest.raises(ValueError, match=r"\[P, 3\] and \[Q, 3\]"):
        uvmap.nearest_neighbours(torch.rand(5, 3), torch.rand(7))


def test_misaligned_views_are_copied(lib_built):
    """The kernels read the table and d enc as 16-byte rows: a view whose storage offset is not a multiple of 4 floats is copied."""
    from texgs import uvmap
    base = torch.zeros(131072 + 1)
    view = base[1:]
    assert view.data_ptr() % 16 != 0
    out = uvmap._aligned(view)
    assert out.data_ptr() % 16 == 0 and torch.equal(out, view)
    ok = torch.zeros(131072)
    assert uvmap._aligned(ok).data_ptr() == ok.data_ptr()


def _proj64(cam, znear, zfar):
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    Pc = torch.zeros(4, 4, dtype=torch.float64)
    Pc[0, 0], Pc[1, 1], Pc[3, 2] = 1 / tx, 1 / ty, 1.0
    Pc[2, 2], Pc[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return Pc


def test_depth2world_inverts_the_projection():
    """depth2world (uv_map_gaussian3d.py:155-165) checked independently: projecting its output with the camera's full projection
    (row-vector convention, clip = [p, 1] @ P) lands on the pixel centres with w = depth."""
    sys.path.insert(0, os.path.join(ROOT, "texture-gs_amd"))
    from texgs import synth
    from texgs.uvmap import depth2world
    cam = synth.fibonacci_cameras(4, 40, 30)[1]
    # the full projection in float64 (synth.projection's matrix, utils/graphics.py:51-71): depth2world rebuilds z_clip from znear /
    # zfar in float64 and does not divide by the homogeneous coordinate, so a float32-rounded P[2,2] would shift points by ~1e-5
    P = cam.world_view_transform.double() @ _proj64(cam, 0.01, 100.0).t()
    depth = torch.rand(30, 40, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 3 + 1
    world = depth2world(depth, P, 100.0, 0.01).reshape(-1, 3)
    clip = torch.cat([world, torch.ones(world.shape[0], 1, dtype=torch.float64)], 1) @ P
    w = clip[:, 3]
    ndc_x = (torch.arange(40, dtype=torch.float64) * 2 + 1) / 40 - 1
    ndc_y = (torch.arange(30, dtype=torch.float64) * 2 + 1) / 30 - 1
    assert torch.allclose(w, depth.reshape(-1), rtol=1e-10, atol=1e-10)
    assert torch.allclose(clip[:, 0] / w, ndc_x.repeat(30), atol=1e-10)
    assert torch.allclose(clip[:, 1] / w, ndc_y.repeat_interleave(40), atol=1e-10)


def test_cpu_tensors_raise(lib_built):
    from texgs import uvmap
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uvmap.hashgrid_encode(torch.rand(4, 3), torch.zeros(131072))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uvmap.InvUVNet()(torch.rand(4, 3), torch.zeros(128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        uvmap.chamfer_distance(torch.rand(1, 5, 3), torch.rand(1, 7, 3))
    with pytest.raises(ValueError, match="batch size 1"):
        uvmap.chamfer_distance(torch.rand(2, 5, 3), torch.rand(2, 7, 3))


def test_uvmap_does_not_import_oracle_or_tests():
    code = ("import sys; sys.path[:0]=[%r]; import texgs.uvmap; "
            "bad = [k for k in sys.modules if k.split('.')[0] in ('oracle', 'tests', 'hashgrid_ref', 'helpers')]; "
            "assert not bad, bad" % os.path.join(ROOT, "texture-gs_amd"))
    subprocess.check_call([sys.executable, "-c", code])


def test_hashgrid_struct_matches_c_layout(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "texture-gs_amd"))
    from texgs import _lib
    consts = {"TEXGS_HASHGRID_MAX_LEVELS": _lib.HASHGRID_MAX_LEVELS, "TEXGS_HASHGRID_FEATURES": _lib.HASHGRID_FEATURES}
    assert abi_check.layout_mismatches("texgs.h", {"TexGSHashGrid": _lib.HashGridStruct}, consts, tmp_path) == []
