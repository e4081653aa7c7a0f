"""The texture-gradient record (csrc/texrec_math.h: rec_word0 / rec_pack / rec_unpack) and the bin reduce's fixed-point scale, stated
in numpy on arrays of bit patterns.

Two kinds of statement live here and the tests use both:
  * the ARITHMETIC, operation by operation (word0, pack, unpack, scale, to_fixed, from_fixed, reduce_bin_fixed): what the compiled
    header is compared with bit for bit;
  * the RULE the format promises, written as value arithmetic in float64 and as predicates (nearest_kept, rule_holds, scale_holds,
    reduce_bin_f64): what the arithmetic itself is held to.  pack_before_fix is the rounding expression the kernels used until the
    NaN fix; on finite inputs the fixed codec must not differ from it in one bit."""
import numpy as np

F, U, I64, F64 = np.float32, np.uint32, np.int64, np.float64
C0 = F(0.28209479177387814)
FX_ONE = 1 << 18
DROP = (5, 5, 4)                   # low mantissa bits each colour channel gives up: cell x, cell y, the high bits of fx18 / fy18
EXP_ONES = 0x7F800000


def bits(v):
    return np.ascontiguousarray(v, F).view(U)


def floats(b):
    return np.ascontiguousarray(b, U).view(F)


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
def word0(fx, fy):
    """-> (w0, hi, fx18, fy18).  The product by 2^18 is exact, so the float32 sum below is the one rounding the kernel makes, fused or
    not; the conversion truncates."""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    with np.errstate(invalid="ignore"):
        qx = np.minimum((fx * F(262144.0) + F(0.5)).astype(U), U(FX_ONE - 1))
        qy = np.minimum((fy * F(262144.0) + F(0.5)).astype(U), U(FX_ONE - 1))
    return (qx & U(0xFFFF)) | (qy << U(16)), (qx >> U(16)) | ((qy >> U(16)) << U(2)), qx, qy


def round_keep(b, drop):
    """the colour word with its `drop` low bits cleared: texrec_math::rec_round"""
    b = np.asarray(b, U)
    mask = U((1 << drop) - 1)
    nonfinite = (b & U(EXP_ONES)) == U(EXP_ONES)
    v = np.where(nonfinite, b | ((b & mask) << U(5)), b + U((1 << drop) >> 1))
    return v & ~mask


def pack_before_fix(b, drop):
    """(bits + half) & ~mask: right for every finite value, wrong for the NaNs whose add carries out of the exponent field"""
    b = np.asarray(b, U)
    return (b + U((1 << drop) >> 1)) & ~U((1 << drop) - 1)


def pack(w0, hi, cx, cy, xb):
    """xb [n, 3] bit patterns -> [n, 4] record words"""
    xb = np.asarray(xb, U)
    out = np.empty((xb.shape[0], 4), U)
    out[:, 0] = w0
    out[:, 1] = round_keep(xb[:, 0], 5) | (np.asarray(cx, U) & U(31))
    out[:, 2] = round_keep(xb[:, 1], 5) | (np.asarray(cy, U) & U(31))
    out[:, 3] = round_keep(xb[:, 2], 4) | np.asarray(hi, U)
    return out


def unpack(w):
    """[n, 4] words -> dict(cx, cy, fx18, fy18, fx, fy (float32), xb [n, 3] bit patterns of the decoded colour)"""
    w = np.asarray(w, U).reshape(-1, 4)
    fx18 = (w[:, 0] & U(0xFFFF)) | ((w[:, 3] & U(3)) << U(16))
    fy18 = (w[:, 0] >> U(16)) | (((w[:, 3] >> U(2)) & U(3)) << U(16))
    xb = np.stack([w[:, 1] & ~U(31), w[:, 2] & ~U(31), w[:, 3] & ~U(15)], 1)
    return dict(cx=(w[:, 1] & U(31)).astype(I64), cy=(w[:, 2] & U(31)).astype(I64), fx18=fx18.astype(I64), fy18=fy18.astype(I64),
                fx=fx18.astype(F) * F(1.0 / 262144.0), fy=fy18.astype(F) * F(1.0 / 262144.0), xb=xb)


def scale(bbits):
    """bits of max |dL/dpixel colour| -> (nonfinite, e, up, down), arrays.  bound = C0 * value in float32, bound < 2^e (frexp; e = 0 for
    a bound of 0), up = 2^(42 - e) and down = 2^(e - 42) in float64."""
    bbits = np.atleast_1d(np.asarray(bbits, U))
    nonfinite = bbits >= U(EXP_ONES)
    with np.errstate(invalid="ignore"):
        bound = C0 * floats(np.where(nonfinite, U(0), bbits))
    _, e = np.frexp(bound)
    e = np.where(nonfinite, 0, e).astype(np.int32)
    up = np.where(nonfinite, 0.0, np.ldexp(F64(1.0), 42 - e))
    down = np.where(nonfinite, 0.0, np.ldexp(F64(1.0), e - 42))
    return nonfinite, e, up, down


def tap_weights(fx, fy):
    """[n] float32 fractions -> [n, 4] float64: each weight one float32 product (1 - fx is exact for a multiple of 2^-18)"""
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    one = F(1.0)
    return np.stack([(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy], 1).astype(F64)


def to_fixed(w, dx):
    """w * dx is a 48-bit product, exact in float64; adding 1.5 * 2^52 rounds it to the nearest integer, ties to even"""
    return np.rint(np.asarray(w, F64) * np.asarray(dx, F64)).astype(I64)


def from_fixed(q, down):
    with np.errstate(under="ignore"):
        return (np.asarray(q, I64).astype(F).astype(F64) * F64(down)).astype(F)


TAP_DY, TAP_DX = (0, 0, 1, 1), (0, 1, 0, 1)


def reduce_bin_fixed(words, bbits):
    """One bin through the reduce's fixed-point path -> the [33, 33, 3] float32 tile the kernel adds to dL_dtexture (finite bound)"""
    nonfinite, _, up, down = scale(bbits)
    assert not nonfinite[0]
    r = unpack(words)
    w = tap_weights(r["fx"], r["fy"])
    dx = floats(r["xb"]).astype(F64) * up[0]
    tile = np.zeros((33, 33, 3), I64)
    for t in range(4):
        np.add.at(tile, (r["cy"] + TAP_DY[t], r["cx"] + TAP_DX[t]), to_fixed(w[:, t, None], dx))
    return from_fixed(tile, down[0])


# ---------------------------------------------------------------------------------------------------------------------- the rule
def nearest_kept(b, drop):
    """The value a FINITE input must decode to, by value arithmetic in float64: the nearest float32 whose `drop` low mantissa bits
    are zero, ties away from zero, the sign kept (of a zero too), inf where that nearest value is 2^128.  -> bit patterns."""
    b = np.asarray(b, U)
    v = floats(b).astype(F64)
    a = np.abs(v)
    _, ex = np.frexp(a)                                        # a in [2^(ex-1), 2^ex)
    step = np.ldexp(F64(1.0), np.maximum(ex - 1, -126) - 23 + drop)        # spacing of the kept values in a's binade (denormals: that of 2^-126)
    q = np.floor(a / step + 0.5) * step                       # a / step < 2^24 and a multiple of 2^-drop: all exact
    with np.errstate(over="ignore"):
        out = bits(np.where(q >= 2.0 ** 128, np.inf, q).astype(F))
    return out | (b & U(0x80000000))


def rule_holds(b, decoded, drop):
    """-> boolean array: the decoded bit pattern is what the format promises for the input bit pattern"""
    b, decoded = np.asarray(b, U), np.asarray(decoded, U)
    mag = b & U(0x7FFFFFFF)
    is_nan, is_inf = mag > U(EXP_ONES), mag == U(EXP_ONES)
    dec_nan = (decoded & U(0x7FFFFFFF)) > U(EXP_ONES)
    low_clear = (decoded & U((1 << drop) - 1)) == 0
    finite_ok = decoded == nearest_kept(np.where(is_nan | is_inf, U(0), b), drop)
    return low_clear & np.where(is_nan, dec_nan, np.where(is_inf, decoded == b, finite_ok))


def scale_holds(bbits):
    """-> list of the bbits (finite) for which the scale breaks its promise: 2^(e-1) <= bound < 2^e, up * down == 1, both finite and
    non-zero; a bound of 0 has e = 0"""
    bbits = np.atleast_1d(np.asarray(bbits, U))
    nonfinite, e, up, down = scale(bbits)
    bound = (C0 * floats(np.where(nonfinite, U(0), bbits))).astype(F64)
    ok = np.isfinite(up) & np.isfinite(down) & (up != 0) & (down != 0) & (up * down == 1.0)
    ok &= np.where(bound == 0, e == 0, (np.ldexp(1.0, e - 1) <= bound) & (bound < np.ldexp(1.0, e)))
    ok &= up == np.ldexp(1.0, 42 - e)
    return [int(x) for x in bbits[~ok & ~nonfinite]]


def reduce_bin_f64(words):
    """One bin in float64 from DECODED records: sum_k w_k x_k per tile texel, w formed exactly from fx18 / fy18 (a 36-bit product).
    -> (tile [33,33,3], n [33,33] contributions, mag [33,33,3] = sum |w x|)"""
    r = unpack(words)
    fx, fy = r["fx18"].astype(F64) / FX_ONE, r["fy18"].astype(F64) / FX_ONE
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    x = floats(r["xb"]).astype(F64)
    tile, mag, n = np.zeros((33, 33, 3)), np.zeros((33, 33, 3)), np.zeros((33, 33), I64)
    for t in range(4):
        at = (r["cy"] + TAP_DY[t], r["cx"] + TAP_DX[t])
        np.add.at(tile, at, w[:, t, None] * x)
        np.add.at(mag, at, np.abs(w[:, t, None] * x))
        np.add.at(n, at, 1)
    return tile, n, mag


def reduce_bar(n, mag, e, roundings=2):
    """n * 2^(e-42) for the roundings to the fixed-point grid + roundings * 2^-24 * sum|w x| (the float32 weight product and the final
    conversion: 2; a seam texel where up to four partial sums meet by float atomics: 3 more)"""
    return n[..., None].astype(F64) * 2.0 ** (int(e) - 42) + roundings * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------- footprints of a blend_ref tile (D3)
def anchor(x0, y0, R):
    """The record convention of render.hip's tap setup (cube_address / tap_binned): a footprint is BINNED when its tap-00 texel
    (x0, y0) lies in [0, R - 2] on both axes -- all four taps are then distinct texels of the face; one clamped at a face border goes
    to dL_dtexture directly and writes no record.  -> (binned, bin y, bin x, cell y, cell x)"""
    binned = (x0 >= 0) & (x0 <= R - 2) & (y0 >= 0) & (y0 <= R - 2)
    return binned, y0 >> 5, x0 >> 5, y0 & 31, x0 & 31
