"""-m "not gpu": the texture-gradient record codec and the bin reduce's fixed-point scale (csrc/texrec_math.h) without a GPU.

The header is what K7 packs with and what k_texgrad_reduce unpacks, scales and converts with; here it is compiled for the host with
g++ -ffp-contract=off into a stand-alone program (input and output through files) and compared bit for bit with the numpy statement
(tests/texrec_ref.py), and the statement's arithmetic is held to the RULE the format promises (round to nearest kept value, ties away
from zero, inf and every NaN kept, a scale for every finite bound).

Two things these tests found in the kernels as they were, both fixed in texrec_math.h:
  * rec_pack rounded with (bits + half) & ~mask on every input: a NaN with mantissa >= 0x7FFFF0 (blue: >= 0x7FFFF8) carried out of the
    exponent field and was stored as +-0.0 -- the rows (exponent 255, mantissa 0x7FFFF0 / 0x7FFFF7 / 0x7FFFF8 / 0x7FFFFF, both signs)
    of test_pack_special_values failed, 0x7FFFF0 and 0x7FFFF7 in red and green only;
  * the scale was formed with the float ldexpf: 2^(42-e) is inf from e = -86 down and 2^(e-42) is 0 from e = -108 down -- test_scale
    failed for every bound below 2^-86 and test_one_bin_reduce at the bounds 2^-140, 2^-126 and 2^-90.
On finite inputs the fixed codec equals the old expression (texrec_ref.pack_before_fix) in every bit; the tests below pin that."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check  # noqa: E402
import texrec_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texture-gs_amd", "csrc")
F, U, I64, F64 = np.float32, np.uint32, np.int64, np.float64

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "texrec_math.h"
namespace tm = texrec_math;
// argv: mode in out.  The input file is uint32 words, the first one n.
//   word0   n fx bits, n fy bits                               -> n w0, n hi
//   pack    n x {w0, hi, cx, cy, x0, x1, x2 bits}              -> n x {a, b, c, d}, n x {cx, cy, fx bits, fy bits, x0, x1, x2 bits}
//   scale   n bbits                                            -> n x {nonfinite, e}, n up (double), n down (double)
//   reduce  n, bbits, n x {a, b, c, d}                         -> 33 x 33 x 3 floats
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 1;
    fseek(f, 0, SEEK_END);
    const size_t bytes = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint32_t> in(bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size() || in.empty()) return 1;
    fclose(f);
    const size_t n = in[0];
    const uint32_t* p = in.data() + 1;
    std::vector<uint32_t> out;
    if (!strcmp(argv[1], "word0")) {
        if (in.size() != 1 + 2 * n) return 3;
        out.resize(2 * n);
        for (size_t i = 0; i < n; ++i) { uint32_t hi; out[i] = tm::rec_word0(tm::float_of(p[i]), tm::float_of(p[n + i]), hi); out[n + i] = hi; }
    } else if (!strcmp(argv[1], "pack")) {
        if (in.size() != 1 + 7 * n) return 3;
        out.resize(11 * n);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t* q = p + 7 * i;
            const tm::Rec4 r = tm::rec_pack(q[0], q[1], (int)q[2], (int)q[3], tm::float_of(q[4]), tm::float_of(q[5]), tm::float_of(q[6]));
            out[4 * i] = r.a; out[4 * i + 1] = r.b; out[4 * i + 2] = r.c; out[4 * i + 3] = r.d;
            const tm::RecVal v = tm::rec_unpack(r);
            uint32_t* o = out.data() + 4 * n + 7 * i;
            o[0] = (uint32_t)v.cx; o[1] = (uint32_t)v.cy; o[2] = tm::bits_of(v.fx); o[3] = tm::bits_of(v.fy);
            o[4] = tm::bits_of(v.x0); o[5] = tm::bits_of(v.x1); o[6] = tm::bits_of(v.x2);
        }
    } else if (!strcmp(argv[1], "scale")) {
        if (in.size() != 1 + n) return 3;
        out.resize(2 * n + 4 * n);
        for (size_t i = 0; i < n; ++i) {
            const tm::Scale s = tm::scale_of(p[i]);
            out[2 * i] = s.nonfinite ? 1u : 0u; out[2 * i + 1] = (uint32_t)s.e;
            memcpy(out.data() + 2 * n + 2 * i, &s.up, 8);
            memcpy(out.data() + 4 * n + 2 * i, &s.down, 8);
        }
    } else if (!strcmp(argv[1], "reduce")) {
        if (in.size() != 2 + 4 * n) return 3;
        const tm::Scale s = tm::scale_of(p[0]);
        if (s.nonfinite) return 4;
        std::vector<long long> tile(33 * 33 * 3, 0ll);
        for (size_t i = 0; i < n; ++i) {
            tm::Rec4 w; w.a = p[1 + 4 * i]; w.b = p[2 + 4 * i]; w.c = p[3 + 4 * i]; w.d = p[4 + 4 * i];
            const tm::RecVal r = tm::rec_unpack(w);
            const double dx[3] = {(double)r.x0 * s.up, (double)r.x1 * s.up, (double)r.x2 * s.up};
            double wt[4];
            tm::tap_weights(r.fx, r.fy, wt);
            for (int t = 0; t < 4; ++t)
                for (int c = 0; c < 3; ++c) tile[((r.cy + (t >> 1)) * 33 + r.cx + (t & 1)) * 3 + c] += tm::to_fixed(wt[t], dx[c]);
        }
        out.resize(tile.size());
        for (size_t i = 0; i < tile.size(); ++i) out[i] = tm::bits_of(tm::from_fixed(tile[i], s.down));
    } else {
        return 2;
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 1;
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("texrec_math")
    src, exe = d / "harness.cpp", d / "harness"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(mode, *arrays):
        words = np.concatenate([np.ascontiguousarray(a).view(U).reshape(-1) for a in arrays])
        (d / "in.bin").write_bytes(words.tobytes())
        subprocess.check_call([str(exe), mode, str(d / "in.bin"), str(d / "out.bin")])
        return np.frombuffer((d / "out.bin").read_bytes(), U)
    return run


def _n(n):
    return np.array([n], U)


# ------------------------------------------------------------------------------------------------------------------- rec_word0
def _word0(harness, fx, fy):
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    out = harness("word0", _n(fx.size), fx, fy)
    w0, hi, qx, qy = T.word0(fx, fy)
    assert np.array_equal(out[:fx.size], w0) and np.array_equal(out[fx.size:], hi)
    # ... and through pack / unpack the 18 bits come back whole
    got = T.unpack(T.pack(w0, hi, 0, 0, np.zeros((fx.size, 3), U)))
    assert np.array_equal(got["fx18"], qx) and np.array_equal(got["fy18"], qy)
    return qx.astype(I64), qy.astype(I64)


def test_word0_every_18_bit_fraction_on_each_axis(harness):
    k = np.arange(T.FX_ONE, dtype=I64)
    exact = (k.astype(F64) / T.FX_ONE).astype(F)              # k / 2^18 is a float32
    zero = np.zeros_like(exact)
    qx, qy = _word0(harness, exact, zero)
    assert np.array_equal(qx, k) and not qy.any()
    qx, qy = _word0(harness, zero, exact)
    assert np.array_equal(qy, k) and not qx.any()


def test_word0_rounds_to_nearest_either_side_of_a_grid_point(harness):
    g = np.random.default_rng(18)
    k = np.unique(np.concatenate([[0, 1, 2, 65535, 65536, 65537, 131071, 131072, 196607, 196608, 262142, 262143],
                                  g.choice(T.FX_ONE, 4096, replace=False)]))
    assert 4096 <= k.size <= 4096 + 12
    for sign in (-1.0, 1.0):
        v = k.astype(F64) / T.FX_ONE + sign * 2.0 ** -20
        v = v[(v >= 0) & (v < 1)]
        f = v.astype(F)
        assert np.array_equal(f.astype(F64), v)                # 18 + 2 bits: exact in float32
        other = np.full_like(f, 0.375)
        for qx, qy, which in (_word0(harness, f, other) + ("x",), _word0(harness, other, f)[::-1] + ("y",)):
            want = np.minimum(np.floor(v * T.FX_ONE + 0.5), T.FX_ONE - 1).astype(I64)
            assert np.array_equal(qx, want), which
            assert np.all(qy == 98304), which
            assert np.all(np.abs(qx / T.FX_ONE - v) <= 2.0 ** -19), which


def test_word0_largest_fraction_below_one_clamps(harness):
    top = np.nextafter(F(1.0), F(0.0))
    qx, qy = _word0(harness, [top, 0.25], [0.25, top])
    assert qx[0] == 262143 and qy[1] == 262143 and qx[1] == 65536 and qy[0] == 65536
    # the one place where the error is 2^-18, not 2^-19: the clamp takes back the round-up to 1
    err = float(top) - 262143 / T.FX_ONE
    assert 2.0 ** -19 < err <= 2.0 ** -18 and err == 2.0 ** -18 - 2.0 ** -24


# ------------------------------------------------------------------------------------------------------- rec_pack / rec_unpack
MANTISSAS = [0, 1, 0xF, 0x10, 0x1F, 0x20, 0x3FFFF0, 0x400000, 0x7FFFE0, 0x7FFFEF, 0x7FFFF0, 0x7FFFF7, 0x7FFFF8, 0x7FFFFF]


def _special_bits():
    e, m, s = np.meshgrid(np.arange(256, dtype=U), np.array(MANTISSAS, U), np.array([0, 1], U), indexing="ij")
    return ((s << U(31)) | (e << U(23)) | m).reshape(-1)


def _pack_round_trip(harness, xb, cell, hi_bits):
    """xb [n] patterns, put in each of the three channel positions in turn (the other two channels hold an unrelated finite value).
    -> for each channel the decoded patterns [n]"""
    n = xb.size
    g = np.random.default_rng(5)
    fx18, fy18 = g.integers(0, T.FX_ONE, n), g.integers(0, T.FX_ONE, n)
    hi = U(hi_bits)
    w0 = ((fx18 & 0xFFFF) | ((fy18 & 0xFFFF) << 16)).astype(U)
    decoded = []
    for ch in range(3):
        x = np.full((n, 3), F(-0.3173).view(U), U)
        x[:, ch] = xb
        rows = np.stack([w0, np.full(n, hi, U), np.full(n, cell, U), np.full(n, 31 - cell, U), x[:, 0], x[:, 1], x[:, 2]], 1)
        out = harness("pack", _n(n), rows)
        words, back = out[:4 * n].reshape(n, 4), out[4 * n:].reshape(n, 7)
        want = T.pack(w0, hi, cell, 31 - cell, x)
        assert np.array_equal(words, want), ch
        u = T.unpack(want)
        # the payload comes back exactly and never leaks into the value
        assert np.all(back[:, 0] == cell) and np.all(back[:, 1] == 31 - cell) and np.all(u["cx"] == cell) and np.all(u["cy"] == 31 - cell)
        assert np.array_equal(u["fx18"], (fx18 & 0xFFFF) | ((int(hi) & 3) << 16)) and np.array_equal(u["fy18"], (fy18 & 0xFFFF) | ((int(hi) >> 2) << 16))
        assert np.array_equal(back[:, 2], T.bits(u["fx"])) and np.array_equal(back[:, 3], T.bits(u["fy"]))
        assert np.array_equal(back[:, 4:7], u["xb"]), ch
        # the value does not depend on the payload beside it
        assert np.array_equal(u["xb"], T.unpack(T.pack(0, 0, 0, 0, x))["xb"]), ch
        decoded.append(u["xb"][:, ch])
    return decoded


@pytest.mark.parametrize("cell,hi", [(0, 0), (31, 15), (0, 15), (31, 0)])
def test_pack_special_values(harness, cell, hi):
    xb = _special_bits()
    assert xb.size == 256 * 14 * 2
    finite = (xb & U(T.EXP_ONES)) != U(T.EXP_ONES)
    for ch, dec in enumerate(_pack_round_trip(harness, xb, cell, hi)):
        drop = T.DROP[ch]
        bad = ~T.rule_holds(xb, dec, drop)
        assert not bad.any(), (ch, [hex(int(b)) for b in xb[bad]][:16], [hex(int(b)) for b in dec[bad]][:16])
        # finite rows: not one bit away from the expression the kernels used before the NaN fix
        assert np.array_equal(dec[finite], T.pack_before_fix(xb[finite], drop)), ch
    # the rule's own edges, by value: a tie goes away from zero; within half a step of overflow decodes to inf; a zero keeps its sign
    one = 0x3F800000
    assert T.nearest_kept(np.array([one | 0x10, one | 0xF, one | 0x8, one | 0x7], U), 5).tolist() == [one | 0x20, one, one, one]
    assert T.nearest_kept(np.array([one | 0x8, one | 0x7, 0x80000000 | one | 0x8], U), 4).tolist() == [one | 0x10, one, 0x80000000 | one | 0x10]
    assert T.nearest_kept(np.array([0x7F7FFFF0, 0x7F7FFFEF, 0xFF7FFFF0, 0x80000000, 0], U), 5).tolist() == [0x7F800000, 0x7F7FFFE0, 0xFF800000, 0x80000000, 0]
    assert T.nearest_kept(np.array([0x7F7FFFF8, 0x7F7FFFF7, 1, 0x10], U), 4).tolist() == [0x7F800000, 0x7F7FFFF0, 0, 0x10]


def test_pack_random_bit_patterns(harness):
    xb = np.random.default_rng(16).integers(0, 2 ** 32, 2 ** 16, dtype=np.uint64).astype(U)
    finite = (xb & U(T.EXP_ONES)) != U(T.EXP_ONES)
    assert 100 < int((~finite).sum()) < 600
    for cell, hi in ((0, 0), (31, 15)):
        for ch, dec in enumerate(_pack_round_trip(harness, xb, cell, hi)):
            assert bool(T.rule_holds(xb, dec, T.DROP[ch]).all()), ch
            assert np.array_equal(dec[finite], T.pack_before_fix(xb[finite], T.DROP[ch])), ch


# --------------------------------------------------------------------------------------------------------------------- the scale
def _scale_bits():
    e = np.arange(256, dtype=U)[:, None] << U(23)
    b = (e | np.array([0, 1, 0x7FFFFF], U)[None]).reshape(-1)
    return np.unique(np.concatenate([b, np.array([1, 2, 4, 0x10, 0x400000, 0x7FFFFF, 0, 0x7F7FFFFF, 0x7F800000, 0x7FC00000], U)]))


def test_scale(harness):
    bb = _scale_bits()
    n = bb.size
    out = harness("scale", _n(n), bb)
    flag, e = out[:2 * n].reshape(n, 2)[:, 0], out[:2 * n].reshape(n, 2)[:, 1].view(np.int32)
    up, down = out[2 * n:4 * n].view(F64), out[4 * n:].view(F64)
    nonfinite, we, wup, wdown = T.scale(bb)
    assert np.array_equal(flag.astype(bool), nonfinite) and np.array_equal(nonfinite, bb >= 0x7F800000)
    fin = ~nonfinite
    assert int(fin.sum()) == 255 * 3 + 4 and np.array_equal(e[fin], we[fin])
    assert np.array_equal(up[fin].view(np.uint64), wup[fin].view(np.uint64)) and np.array_equal(down[fin].view(np.uint64), wdown[fin].view(np.uint64))
    assert T.scale_holds(bb) == []
    # the ends of the range: the smallest bound that C0 does not round to 0, and the largest
    assert int(we[bb == 1][0]) == 0                            # C0 * 2^-149 rounds to 0
    assert int(we[bb == 0x7F7FFFFF][0]) == 127 and int(we[bb == 0][0]) == 0
    assert int(we[bb == 4][0]) == -148 and int(we[bb == 0x7FFFFF][0]) == -127   # denormal bounds
    # a bound of 0: every record of such a call is 0 and so is every contribution
    z = T.reduce_bin_fixed(T.pack(0x80008000, 5, 3, 4, np.zeros((1, 3), U)), 0)
    assert not z.any()


# ------------------------------------------------------------------------------------------------------------- the one-bin reduce
BOUNDS = [-140, -126, -90, -86, -85, 0, 100, 126]


def _records(seed, bound_exp, n=1000):
    """n records of one bin with values up to the bound 2^bound_exp (C0 * max|dL/dpixel| = 2^bound_exp exactly is no float product,
    so the bound's bits are those of the smallest max|dL/dpixel| whose bound is >= 2^bound_exp)"""
    g = np.random.default_rng(seed)
    target = F64(2.0) ** bound_exp
    m = F(target / F64(T.C0))
    while F64(T.C0 * m) < target:
        m = np.nextafter(m, F(np.inf))
    bbits = int(F(m).view(U))
    bound = F64(T.C0 * m)
    x = (g.uniform(-1.0, 1.0, (n, 3)) * bound).astype(F)
    x[::17] = (np.sign(x[::17]).astype(F64) * bound).astype(F)                 # some at the bound itself
    x[5::29, 1] = 0.0
    cx, cy = g.integers(0, 32, n), g.integers(0, 32, n)
    cx[:40], cy[:40] = 7, 9                                    # one cell hit 40 times and its neighbours often
    cx[40:60], cy[40:60] = 31, 31                              # the tile's 33rd row and column
    fx18, fy18 = g.integers(0, T.FX_ONE, n), g.integers(0, T.FX_ONE, n)
    fx18[60:70], fy18[60:70] = 0, T.FX_ONE - 1
    w0, hi, _, _ = T.word0((fx18 / T.FX_ONE).astype(F), (fy18 / T.FX_ONE).astype(F))
    return T.pack(w0, hi, cx, cy, T.bits(x)), bbits


@pytest.mark.parametrize("bound_exp", BOUNDS)
def test_one_bin_reduce(harness, bound_exp):
    """1000 records through the header's fixed-point path: bit for bit the statement's, and within the derived bar of the float64
    sum: n * 2^(e-42) for the roundings to the grid + 2 * 2^-24 * sum|w x| (the float32 weight product, the final conversion)"""
    words, bbits = _records(1000 + bound_exp, bound_exp)
    _, e, up, down = T.scale(bbits)
    assert int(e[0]) == bound_exp + 1 and np.isfinite(up[0]) and down[0] > 0
    out = harness("reduce", _n(words.shape[0]), np.array([bbits], U), words).view(F).reshape(33, 33, 3)
    want = T.reduce_bin_fixed(words, bbits)
    assert np.array_equal(out.view(U), want.view(U))
    ref, n, mag = T.reduce_bin_f64(words)
    assert int(n.max()) >= 40 and int(n[32].sum()) > 0 and int(n[:, 32].sum()) > 0
    bar = T.reduce_bar(n, mag, int(e[0]))
    # the final conversion's rounding is half a step of the float32 RESULT: 2^-24 relative (in the bar) for a normal one, 2^-150 absolute
    # where the sum itself is below 2^-126 and no float32 can come closer (texels of the bounds 2^-126 and 2^-140 only)
    tiny = (np.abs(ref) < 2.0 ** -126) & (mag > 0)
    assert bound_exp <= -126 or not tiny.any()
    bar = bar + np.where(tiny, 2.0 ** -150, 0.0)
    d = np.abs(out.astype(F64) - ref)
    assert not d[bar == 0].any()
    over = float((d[bar > 0] / bar[bar > 0]).max())
    print(f"texrec/one_bin_reduce bound 2^{bound_exp}: worst error / bar = {over:.3f}")
    assert over <= 1.0
    assert np.abs(ref).max() > 0.5 * 2.0 ** bound_exp           # (the sums are of the bound's size: a bar that passes zeros would not do)


def test_header_is_listed_and_stands_alone(tmp_path):
    abi_check.build_knows_header(os.path.join(CSRC, "texrec_math.h"))
    render = open(os.path.join(CSRC, "render.hip")).read()
    assert '#include "texrec_math.h"' in render
    for gone in ("uint32_t rec_word0(", "Rec4 rec_pack(", "RecVal rec_unpack(", "ldexpf("):
        assert gone not in render, gone                        # stated once, in the header
    src = tmp_path / "alone.cpp"
    src.write_text('#include "texrec_math.h"\nint main() { return (int)texrec_math::scale_of(0u).e; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-I", CSRC, str(src), "-o", str(tmp_path / "alone")])
