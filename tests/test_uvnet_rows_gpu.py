"""The UV-net kernels (csrc/uvnet.hip) row by row and entry by entry against the float64 statement of tests/uvnet_ref.py.

Forward (texgs_uv_pack + texgs_uv_taylor_packed through ctypes): EVERY row of uvs and of J, error of a row = max |difference| over
the row / max |reference| of the row.  On the probe networks the matrix products are exact, so the only arithmetic left is the
normalise step: the bar is 4 x the largest row error of the float32 statement's normalise step on the same exact o, dO (over the
probe's 129 inputs, of which every size is a prefix), floored at 2^-24, the precisions must agree bit for bit, and the fp32 kernel's
bits are those of the float32 normalise step in uv_finish's own operation order.  On random and ill-scaled nets the bar is 4 x the
error of the float32 statement with the same split planes.

Backward (texgs_uv_backward through ctypes, so NULL pointers get there): EVERY entry of the ten gradients, error of an entry in units
of its own scale S (uvnet_ref.backward), bar 4 x the largest such figure of the float32 statement over the ten, floored at 2^-24; one
launch per point position of a tile, each under the bar of its own point; NULL inputs and outputs; guard words.

Off the probes the float32 statement's figure is the larger of two summation orders (uvnet_ref.reordered).

The figures come from the `figures_*` functions (scripts/uvnet_rows_parity.py records them in profiles/uvnet_rows_parity.json); the
tests assert on them."""
import functools

import pytest
import torch

import uvnet_ref as R

PRECISIONS = ("fp32", "mixed", "bf16x3")
PROBE_SIZES = (1, 31, 32, 33, 97, 129)             # a forward tile is 32 points
BACKWARD_SIZES = (1, 63, 64, 65, 200, 16_385, 16_450)      # a backward tile is 64 points, the grid at most 256 workgroups
F32, F64 = torch.float32, torch.float64


def _floored(e):
    return max(float(e), R.FLOOR)


# ------------------------------------------------------------------------------------------------------------------ forward
@functools.lru_cache(maxsize=None)
def _probe_reference(kind, bias, norm):
    """Once per probe: inputs, float64 uvs / J, the float32 normalise step's row errors, and per precision whether the float32 statement
    with that precision's split planes reproduces float64's o / dO bit for bit (then so must the kernel) or else its own row errors."""
    net, emb = R.probe(kind, bias, norm)
    xyz = R.probe_points(kind, bias, norm, max(PROBE_SIZES))
    o, dO, _ = R.sums(net, emb, xyz, F64)
    uv64, J64 = R.finish(o, dO, F64)
    uv32, J32 = R.finish(o, dO, F32)
    ref = {"net": net, "emb": emb, "xyz": xyz, "uvs": uv64, "J": J64, "step": (R.row_error(uv32, uv64), R.row_error(J32, J64)), "planes": {},
           "kernel_order": R.finish_kernel_order(o, dO)}
    for prec in PRECISIONS:
        os_, ds_, _ = R.sums(net, emb, xyz, F32, R.SPLIT_PLANES[prec])
        us, Js = R.finish(os_, ds_, F32)
        ref["planes"][prec] = {"exact_o": torch.equal(os_.double(), o), "exact_dO": torch.equal(ds_.double(), dO),
                               "rows": (R.row_error(us, uv64), R.row_error(Js, J64))}
    return ref


def figures_probe_forward(kind, bias, norm, n):
    """One size of one probe in the three precisions -> per precision the worst row of uvs and of J (error, row index), the bar's
    yardstick and the ratio, whether the rows past N kept their fill, and the bit identities between the precisions."""
    import uvnet_raw as D
    ref = _probe_reference(kind, bias, norm)
    out, got = {"probe": kind, "bias": bias, "norm": norm, "N": n, "precision": {}}, {}
    for prec in PRECISIONS:
        uvs, J = D.forward(ref["net"], ref["emb"], ref["xyz"][:n], prec)
        fig = {"rows_past_N_untouched": bool((uvs[n:] == D.SENTINEL).all()) and bool((J[n:] == D.SENTINEL).all())}
        got[prec] = (uvs[:n], J[:n])
        pl = ref["planes"][prec]
        for name, g, want, step, rows, exact in (("uvs", uvs[:n], ref["uvs"][:n], ref["step"][0], pl["rows"][0], pl["exact_o"]),
                                                 ("J", J[:n], ref["J"][:n], ref["step"][1], pl["rows"][1], pl["exact_o"] and pl["exact_dO"])):
            e = R.row_error(g, want)
            yard = _floored((step if exact else rows).max())
            fig[name] = {"exact_products": exact, "device_error": float(e.max()), "worst_row": int(e.argmax()),
                         "float32_statement_error_floored": yard, "ratio": float(e.max()) / yard}
        out["precision"][prec] = fig
    pl = ref["planes"]
    # the fp32 kernel's o / dO are exact on every probe, and uv_finish is one function of them: its bits are those of the float32 statement of
    # the normalise step in uv_finish's own operation order (torch's division-based R.finish rounds elsewhere; that one is held to the bar)
    ku, kJ = ref["kernel_order"]
    ident = {"fp32_uvs_equal_statement_in_kernel_order": R.same_bits(got["fp32"][0], ku[:n]),
             "fp32_J_equal_statement_in_kernel_order": R.same_bits(got["fp32"][1], kJ[:n]),
             "mixed_uvs_equal_fp32": R.same_bits(got["mixed"][0], got["fp32"][0])}
    if pl["mixed"]["exact_dO"]:
        ident["mixed_J_equal_fp32"] = R.same_bits(got["mixed"][1], got["fp32"][1])
    if pl["bf16x3"]["exact_o"]:
        ident["bf16x3_uvs_equal_fp32"] = R.same_bits(got["bf16x3"][0], got["fp32"][0])
        if pl["bf16x3"]["exact_dO"]:
            ident["bf16x3_J_equal_fp32"] = R.same_bits(got["bf16x3"][1], got["fp32"][1])
    out["bit_identities"] = ident
    out["largest_ratio"] = max(f[k]["ratio"] for f in out["precision"].values() for k in ("uvs", "J"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("kind", R.PROBE_KINDS)
def test_exact_probes_every_row(lib_built, kind, bias, norm):
    """Probes A and B (one wide layer each: B2, B3, B4), with and without biases (NULL pointers) and offset / scale (NULL pointers),
    N = 1 ... 129 in all three precisions.  Where the statement says a precision's products are exact on the probe -- all of probe A,
    the f32 planes of probe B, and its split planes where no low half meets a low half -- uvs and J must be within 4 x the float32
    normalise step of float64 at EVERY row and bit-identical to the fp32 kernel's; elsewhere within 4 x the float32 statement with
    that precision's split planes.  Rows past N keep their fill."""
    ref = _probe_reference(kind, bias, norm)
    if kind == "A":
        assert all(p["exact_o"] and p["exact_dO"] for p in ref["planes"].values())
    assert ref["planes"]["fp32"]["exact_o"] and ref["planes"]["fp32"]["exact_dO"] and ref["planes"]["mixed"]["exact_o"]
    for n in PROBE_SIZES:
        fig = figures_probe_forward(kind, bias, norm, n)
        print(fig)
        for prec, f in fig["precision"].items():
            assert f["rows_past_N_untouched"], (n, prec)
            for name in ("uvs", "J"):
                assert f[name]["ratio"] <= R.BAR, (n, prec, name, f[name])
        assert all(fig["bit_identities"].values()), (n, fig["bit_identities"])
        if kind == "A":
            assert len(fig["bit_identities"]) == 6


@functools.lru_cache(maxsize=None)
def _net(which):
    """(Net, emb, the Net whose kinks choose the inputs, its emb): (a) a fresh init, (b) the golden net, (c) net (a) with rows 2^-6 ... 2^6."""
    if which == "golden":
        net, emb, _ = R.golden_net()
        return net, emb, net, emb
    net, emb = R.fresh_net(11, True)
    if which == "rescaled":          # the same function and, row by row, the same roundings times a power of two: net (a)'s safe points
        return R.rescaled(net, emb) + (net, emb)
    return net, emb, net, emb


@functools.lru_cache(maxsize=None)
def _random_reference(which, n, margin, planes):
    net, emb, sel, sel_emb = _net(which)
    xyz = R.safe_points(sel, sel_emb, n, margin)
    uv64, J64 = R.forward(net, emb, xyz, F64)
    e_uv, e_J = _statement_rows(net, emb, xyz, planes, uv64, J64)
    return xyz, uv64, J64, _floored(e_uv.max()), _floored(e_J.max()), e_J


def _statement_rows(net, emb, xyz, planes, uv64, J64):
    """Per row the float32 statement's error of uvs and of J, the larger of two summation orders (R.reordered: the host's float32 error
    is one draw per order)."""
    net2, emb2, _ = R.reordered(net, emb)
    (ua, Ja), (ub, Jb) = R.forward(net, emb, xyz, F32, planes), R.forward(net2, emb2, xyz, F32, planes)
    return torch.maximum(R.row_error(ua, uv64), R.row_error(ub, uv64)), torch.maximum(R.row_error(Ja, J64), R.row_error(Jb, J64))


def figures_random_forward(which, n):
    import uvnet_raw as D
    net, emb, _, _ = _net(which)
    out, got = {"net": which, "N": n, "precision": {}}, {}
    for prec in PRECISIONS:
        margin = 1e-3 if prec == "bf16x3" else 1e-5
        xyz, uv64, J64, y_uv, y_J, _ = _random_reference(which, n, margin, R.SPLIT_PLANES[prec])
        uvs, J = D.forward(net, emb, xyz, prec)
        got[prec] = uvs[:n]
        e_uv, e_J = R.row_error(uvs[:n], uv64), R.row_error(J[:n], J64)
        out["precision"][prec] = {
            "rows_past_N_untouched": bool((uvs[n:] == D.SENTINEL).all()) and bool((J[n:] == D.SENTINEL).all()),
            "uvs": {"device_error": float(e_uv.max()), "worst_row": int(e_uv.argmax()), "float32_statement_error_floored": y_uv, "ratio": float(e_uv.max()) / y_uv},
            "J": {"device_error": float(e_J.max()), "worst_row": int(e_J.argmax()), "float32_statement_error_floored": y_J, "ratio": float(e_J.max()) / y_J}}
    out["bit_identities"] = {"mixed_uvs_equal_fp32": R.same_bits(got["mixed"], got["fp32"])}
    out["largest_ratio"] = max(f[k]["ratio"] for f in out["precision"].values() for k in ("uvs", "J"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 200])
@pytest.mark.parametrize("which", ["fresh", "golden", "rescaled"])
def test_random_and_ill_scaled_nets_every_row(lib_built, which, n):
    """A fresh init, the reference's golden net, and the fresh net with the rows of W2..W4 up to 4096 x apart (as trained nets are: a
    whole-tensor L2 is blind to the small rows): ALL rows of uvs and J within 4 x the float32 statement with the same split planes;
    inputs from safe_points (margin 1e-5, 1e-3 where the value column is split); "mixed" has the fp32 kernel's uvs bit for bit."""
    fig = figures_random_forward(which, n)
    print(fig)
    for prec, f in fig["precision"].items():
        assert f["rows_past_N_untouched"], prec
        for name in ("uvs", "J"):
            assert f[name]["ratio"] <= R.BAR, (prec, name, f[name])
    assert fig["bit_identities"]["mixed_uvs_equal_fp32"]


RAGGED_SUBSETS = [slice(0, n) for n in (1, 31, 32, 33, 64, 65)] + [slice(5, 70), slice(0, 97)]


def figures_ragged_J(prec):
    import uvnet_raw as D
    net, emb, _, _ = _net("fresh")
    xyz, _, J64, _, _, rows = _random_reference("fresh", 97, 1e-3, R.SPLIT_PLANES[prec])
    out = {"precision": prec, "subsets": []}
    for sl in RAGGED_SUBSETS:
        n = sl.stop - sl.start
        _, J = D.forward(net, emb, xyz[sl], prec)
        e = R.row_error(J[:n], J64[sl])
        yard = _floored(rows[sl].max())
        out["subsets"].append({"rows": [sl.start, sl.stop], "device_error": float(e.max()), "worst_row": sl.start + int(e.argmax()),
                               "float32_statement_error_floored": yard, "ratio": float(e.max()) / yard,
                               "rows_past_N_untouched": bool((J[n:] == D.SENTINEL).all())})
    out["largest_ratio"] = max(s["ratio"] for s in out["subsets"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECISIONS)
def test_ragged_tiles_J_against_float64(lib_built, prec):
    """The subsets and sizes of test_uvnet.py::test_ragged_tiles_depend_on_their_own_point_only (prefixes of 1, 31, 32, 33, 64, 65
    points, the slice 5:70 and all 97), where J was only ever compared with other launches of the same kernel: every row of J of
    every launch against float64, the bar from the float32 statement on the rows of that launch."""
    fig = figures_ragged_J(prec)
    print(fig)
    for s in fig["subsets"]:
        assert s["rows_past_N_untouched"] and s["ratio"] <= R.BAR, s


# ------------------------------------------------------------------------------------------------------------------ backward
def _bw_net(which):
    if which == "probeA":
        return R.probe("A", True, True)
    return _net(which)[:2]


@functools.lru_cache(maxsize=None)
def _bw_inputs(which, n):
    if which == "probeA":            # its forward is exact: no mask is in doubt, no input selection
        xyz = R.probe_points("A", True, True, n)
    else:
        xyz = R.safe_points(*_net(which)[2:], n, 1e-5, seed=n)
    g = torch.randn(n, 3, generator=torch.Generator().manual_seed(100 + n)).double()
    return xyz, g


@functools.lru_cache(maxsize=None)
def _bw_reference(which, n):
    """Shared by the precisions: float64 gradients and scales, and the float32 statement's largest entry error plain and split."""
    net, emb = _bw_net(which)
    xyz, g = _bw_inputs(which, n)
    ref, S, _ = R.backward(net, emb, xyz, g, F64, scales=True)
    return ref, S, {split: _statement_errors(net, emb, xyz, g, ref, S, split) for split in (False, True)}


def _statement_errors(net, emb, xyz, g, ref, S, split):
    """Per output the float32 statement's largest entry error, the larger of two summation orders (the host's float32 error is one
    draw per order; one draw alone makes a bar that moves with the host's matmul)."""
    a, b = R.backward(net, emb, xyz, g, F32, split=split), R.backward_reordered(net, emb, xyz, g, F32, split=split)
    return {k: max(R.entry_error(a[k], ref[k], S[k]), R.entry_error(b[k], ref[k], S[k])) for k in R.NAMES}


def _entry_figures(got, ref, S, yard):
    fig = {k: {"device_error": R.entry_error(got[k], ref[k], S[k]), "worst_entry": list(R.worst_entry(got[k], ref[k], S[k])),
               "float32_statement_error": yard[k]} for k in R.NAMES}
    y = _floored(max(yard.values()))
    worst = max(R.NAMES, key=lambda k: fig[k]["device_error"])
    return {"outputs": fig, "float32_statement_error_floored": y, "worst_output": worst, "device_error": fig[worst]["device_error"],
            "ratio": fig[worst]["device_error"] / y}


def figures_backward(which, n, prec):
    import uvnet_raw as D
    net, emb = _bw_net(which)
    xyz, g = _bw_inputs(which, n)
    ref, S, yard = _bw_reference(which, n)
    got, clean = D.backward(net, emb, xyz, g, prec)
    again, _ = D.backward(net, emb, xyz, g, prec)
    fig = _entry_figures(got, ref, S, yard[prec != "fp32"])
    fig.update({"net": which, "N": n, "precision": prec, "guards_untouched": clean,
                "repeat_is_bit_identical": all(R.same_bits(got[k], again[k]) for k in R.NAMES)})
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("n", BACKWARD_SIZES)
@pytest.mark.parametrize("which", ["probeA", "fresh", "rescaled"])
def test_backward_every_entry(lib_built, which, n, prec):
    """Every entry of the ten gradients, |device - float64| in units of the entry's own scale, within 4 x the float32 statement's
    largest such figure (the six products of the backward chain split where the kernel splits them).  Sizes: a point, around one tile,
    a ragged tail, one point past 256 tiles (workgroup 0 owns a second tile) and workgroup 1's second tile ragged.  "bf16x3" takes the
    split backward through the ABI's "not FP32".  A second launch returns the same bits (no atomics)."""
    fig = figures_backward(which, n, prec)
    print({k: v for k, v in fig.items() if k != "outputs"}, {k: v["device_error"] for k, v in fig["outputs"].items()})
    assert fig["guards_untouched"] and fig["repeat_is_bit_identical"]
    assert fig["ratio"] <= R.BAR, (fig["worst_output"], fig["outputs"][fig["worst_output"]], fig["float32_statement_error_floored"])


SWEEP_TAIL = tuple(range(16_384, 16_448))        # workgroup 0's second tile: its first point 16 384, odd in-pair 16 391, mid-stage 16 415, last 16 447


def figures_position_sweep(which, prec, n, positions):
    """g non-zero at ONE point p per launch: the gradients are that point's contribution.  -> per p the entry figures against the
    float64 statement on that point alone, and the count of entries that are exactly zero in float64 but not on the device."""
    import uvnet_raw as D
    net, emb = _bw_net(which)
    xyz, g = _bw_inputs(which, n)
    out = {"net": which, "precision": prec, "N": n, "positions": []}
    for p in positions:
        gp = torch.zeros_like(g)
        gp[p] = g[p]
        got, clean = D.backward(net, emb, xyz, gp, prec)
        ref, S, _ = R.backward(net, emb, xyz[p:p + 1], g[p:p + 1], F64, scales=True)
        fig = _entry_figures(got, ref, S, _statement_errors(net, emb, xyz[p:p + 1], g[p:p + 1], ref, S, prec != "fp32"))
        out["positions"].append({"p": p, "guards_untouched": clean, "worst_output": fig["worst_output"],
                                 "worst_entry": fig["outputs"][fig["worst_output"]]["worst_entry"], "device_error": fig["device_error"],
                                 "float32_statement_error_floored": fig["float32_statement_error_floored"], "ratio": fig["ratio"],      # the bar of THIS launch
                                 "nonzero_where_float64_is_zero": int(sum(int(((ref[k] == 0) & (got[k].double() != 0)).sum()) for k in R.NAMES)),
                                 "float64_zero_entries": int(sum(int((ref[k] == 0).sum()) for k in R.NAMES))})
    out["largest_ratio"] = max(f["ratio"] for f in out["positions"])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "mixed"])
@pytest.mark.parametrize("which", ["probeA", "fresh"])
def test_backward_point_positions(lib_built, which, prec):
    """One launch per point position of a tile (N = 64, p = 0 ... 63), and at N = 16 448 per position of the wrapped tile (its first
    point, odd in-pair positions, mid-stage positions, the last point): with g non-zero at p alone the ten gradients are that one point's terms, entry
    by entry under the bar of its own launch (4 x the float32 statement on that one point), and every entry that is exactly zero in float64 (a dead unit's row or column) is exactly zero.  What
    sees a wrong stage of bw_outer / bw_outer_b16 (stage q = 4 sk + t reads points 16 sk ... 16 sk + 15) or of bw_gemm_b16."""
    for n, positions in ((64, range(64)), (16_448, SWEEP_TAIL)):
        fig = figures_position_sweep(which, prec, n, list(positions))
        for f in fig["positions"]:
            assert f["float64_zero_entries"] > 0
            assert f["guards_untouched"] and f["nonzero_where_float64_is_zero"] == 0, (n, f)
            assert f["ratio"] <= R.BAR, (n, f)
        print(n, {f["p"]: round(f["ratio"], 3) for f in fig["positions"]})


def figures_null_handling(prec, n=200):
    import uvnet_raw as D
    net, emb = R.fresh_net(11, True)
    xyz, g = _bw_inputs("fresh", n)
    bare = net.without_bias().without_norm()
    got_null, clean0 = D.backward(bare, emb, xyz, g, prec)
    got_zero, clean1 = D.backward(bare.with_zero_bias().with_unit_norm(), emb, xyz, g, prec)
    full, clean2 = D.backward(net, emb, xyz, g, prec)
    out = {"precision": prec, "N": n, "guards_untouched": clean0 and clean1 and clean2,
           "null_inputs_equal_zero_bias_unit_scale": all(R.same_bits(got_null[k], got_zero[k]) for k in R.NAMES), "null_output": {}}
    for name in R.NAMES:
        got, clean = D.backward(net, emb, xyz, g, prec, null_outputs=(name,))
        out["null_output"][name] = clean and got[name] is None and all(R.same_bits(got[k], full[k]) for k in R.NAMES if k != name)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_backward_null_pointers(lib_built, prec):
    """NULL b1..b5 and NULL offset / scale give the bits of zero biases and offset 0 / scale 1; each output pointer NULL in turn leaves
    the other nine bit-identical to the full call ("a NULL pointer skips that gradient"); the guard words around every output buffer
    keep their fill."""
    fig = figures_null_handling(prec)
    print(fig)
    assert fig["guards_untouched"] and fig["null_inputs_equal_zero_bias_unit_scale"]
    assert all(fig["null_output"].values()), fig["null_output"]
