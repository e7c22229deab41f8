"""Analytic known-answer tests for the oracle's CLAHE trio (musica_oracle_k_clahe_histogram / _grad_curve / _grad_curve_apply).

The reference keeps CLAHE behind a disabled #ifdef and the three shaders are not hosted against their text (clahe_grad_curve_apply.comp
reads one past its array), so the oracle's reading of them is pinned here: every expected value is worked out by hand from the shader's
arithmetic, in exact fractions, on inputs whose results are dyadic (so "expected" is an exact float32), with the derivation next to it.
Shader lines are cited as file:line. Two decisions the shaders leave open are the project's (csrc/kernels_clahe.hip, header comment) and
are pinned as such: uint() of a negative tile coordinate saturates to 0, and points[256], one past a tile's curve, reads as (0, 0).

Layout everywhere: hist[tx][ty][bin] and points[tx][ty][i], tx from the column x, ty from the row y; numpy images are [y][x]."""
import math
from fractions import Fraction

import numpy as np
import pytest

T, B = 4, 256
F = np.float32


def _tile_exact(v, n):
    """uint(float(v) / float(n) * 4) (clahe_histogram.comp:34-35) in exact arithmetic."""
    return (4 * v) // n


def _hist_of(ob, img, relevant=None):
    img = np.asarray(img, dtype=F)
    return ob.k_clahe_histogram(img, np.ones_like(img) if relevant is None else relevant)


# ---- clahe_histogram.comp ---------------------------------------------------------------------------------------------------------------

# scaled = v * 255 + 0.5, bin = int(scaled) (:20): 0 -> 0.5 -> 0; 1/8 -> 32.375 -> 32; 1/2 -> 128.0 -> 128; 1 -> 255.5 -> 255. A side that is a
# multiple of 4 puts x / N * 4 on an exact k at every tile border, so each of the 16 tiles holds (N / 4)^2 texels.
@pytest.mark.parametrize("side", [4, 8, 12, 20])
@pytest.mark.parametrize("v,bin_", [(0.0, 0), (0.125, 32), (0.5, 128), (1.0, 255)])
def test_histogram_of_a_constant_image(ob, side, v, bin_):
    h = _hist_of(ob, np.full((side, side), v))
    want = np.zeros((T, T, B), dtype=np.uint32)
    want[:, :, bin_] = (side // 4) ** 2
    assert np.array_equal(h, want)


# v = k / 256 (k < 128): scaled = k - k/256 + 1/2, exact in float32 and inside (k, k + 1): bin k. With v[y][x] = x / 256 the bin names the
# column, so hist[tx][ty][x] = #rows of tile ty where tx = floor(4 x / N) and 0 elsewhere; v[y][x] = y / 256 does the same for the rows. 4 v / N is
# an integer only at v = 0 (and N / 2 for even N), where the float quotient is exact; every other quotient is at least 1 / N from an integer.
@pytest.mark.parametrize("side", [5, 7, 10, 13, 83, 90])
def test_histogram_tile_of_every_column_and_row_at_ragged_sides(ob, side):
    assert side < 128
    idx = np.arange(side)
    tiles = [_tile_exact(int(v), side) for v in idx]
    per_tile = [tiles.count(t) for t in range(T)]
    assert sum(per_tile) == side and max(tiles) == T - 1
    ramp = (idx / 256.0).astype(F)
    by_col = _hist_of(ob, np.tile(ramp, (side, 1)))
    by_row = _hist_of(ob, np.tile(ramp[:, None], (1, side)))
    want_col = np.zeros((T, T, B), dtype=np.uint32)
    want_row = np.zeros((T, T, B), dtype=np.uint32)
    for v in idx:
        want_col[tiles[v], :, v] = per_tile          # column v: tile tx = tiles[v], one texel per row, rows split over the ty
        want_row[:, tiles[v], v] = per_tile          # row v: tile ty = tiles[v], columns split over the tx
    assert np.array_equal(by_col, want_col)
    assert np.array_equal(by_row, want_row)


# relevantPixel == 1.0 (:39) and nothing else: the ramp of img_relevant.comp gives values just under 1, which do not count.
def test_histogram_counts_only_texels_whose_relevant_value_is_exactly_one(ob):
    side = 8
    img = np.full((side, side), 0.5, dtype=F)
    rel = np.zeros((side, side), dtype=F)
    others = [0.0, 0.999, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)), 2.0, -1.0, np.nan, np.inf, 0.5, (5.999 / 6.0) ** 5]
    rel.flat[:len(others)] = others                  # rows 0 and 1
    rel[5, 2] = 1.0                                  # tile (1, 2)
    rel[6, 7] = 1.0                                  # tile (3, 3)
    rel[7, 7] = 1.0
    want = np.zeros((T, T, B), dtype=np.uint32)
    want[1, 2, 128] = 1
    want[3, 3, 128] = 2
    assert np.array_equal(ob.k_clahe_histogram(img, rel), want)


def _bin_in_float64(v):
    """int(v * 255 + 0.5) with each float32 rounding made explicit: a float32 times 255 and a float32 plus 0.5 are exact in float64."""
    scaled = F(np.float64(F(np.float64(v) * 255.0)) + 0.5)
    return int(scaled) if -1.0 < scaled < 256.0 else None


_EDGE = F(255.5 / 255.0)   # v * 255 + 0.5 crosses 256 here
# int() truncates towards zero, so scaled in (-1, 0) is bin 0 (:20, :42): -1/256 -> -255/256 + 1/2 = -127/256 -> 0; -3/512 -> -0.994.. -> 0;
# -1/128 -> -1.4921875 -> -1: outside the image, dropped. 513/512 -> 255.998046875 -> 255; 257/256 -> 256.49609375 -> 256: dropped.
# NaN, +-inf and values whose scaled does not fit an int index nothing (oracle rule Q6).
@pytest.mark.parametrize("v,bin_", [(0.0, 0), (-0.0, 0), (1 / 512, 0), (1 / 256, 1), (-1 / 256, 0), (-3 / 512, 0), (-1 / 128, None), (-0.25, None),
                                    (1.0, 255), (513 / 512, 255), (257 / 256, None), (1.5, None), (np.nan, None), (np.inf, None), (-np.inf, None),
                                    (1e7, None), (-1e30, None), (3e38, None)]
                         + [(float(np.nextafter(_EDGE, F(0)) if d < 0 else _EDGE if d == 0 else np.nextafter(_EDGE, F(2))), "f64") for d in (-1, 0, 1)]
                         + [(float(F(_EDGE - 4e-7)), "f64"), (float(F(_EDGE + 4e-7)), "f64")])
def test_histogram_bin_edges_and_dropped_values(ob, v, bin_):
    if bin_ == "f64":
        bin_ = _bin_in_float64(F(v))
    h = _hist_of(ob, np.full((4, 4), v))             # side 4: one texel per tile
    want = np.zeros((T, T, B), dtype=np.uint32)
    if bin_ is not None:
        want[:, :, bin_] = 1
    assert np.array_equal(h, want)


def test_the_float64_bin_rule_sees_both_sides_of_the_upper_edge():
    """The five values around (256 - 0.5) / 255 above really straddle the edge: the lower ones count in bin 255, the upper ones are dropped."""
    got = [_bin_in_float64(F(v)) for v in (F(_EDGE - 4e-7), np.nextafter(_EDGE, F(0)), _EDGE, np.nextafter(_EDGE, F(2)), F(_EDGE + 4e-7))]
    assert got[0] == 255 and got[-1] is None and set(got) == {255, None}
    assert _bin_in_float64(F(513 / 512)) == 255 and _bin_in_float64(F(257 / 256)) is None and _bin_in_float64(F(-1 / 256)) == 0


# Four quadrants with four bins (1/8 -> 32, 1/4 -> 64.25 -> 64, 1/2 -> 128, 3/4 -> 191.75 -> 191): the right top quadrant is tx >= 2, ty < 2
# (:34-35, :42: ivec3(tilePosX, tilePosY, bin)). Transposing the tile index swaps bins 64 and 128.
def test_histogram_layout_is_tx_ty_bin(ob):
    side, g = 8, 2
    img = np.empty((side, side), dtype=F)
    img[:4, :4], img[:4, 4:], img[4:, :4], img[4:, 4:] = 0.125, 0.25, 0.5, 0.75
    want = np.zeros((T, T, B), dtype=np.uint32)
    want[:2, :2, 32] = g * g
    want[2:, :2, 64] = g * g
    want[:2, 2:, 128] = g * g
    want[2:, 2:, 191] = g * g
    assert np.array_equal(_hist_of(ob, img), want)


# ---- clahe_grad_curve.comp --------------------------------------------------------------------------------------------------------------

def _abscissae():
    x = np.arange(B, dtype=np.float64) / B           # :87 i * (1 / 256)
    x[B - 1] = 1.0                                   # :90
    return x.astype(F)


def _curve_expected(kind, arg):
    """(counts[256], ordinates[256] as exact Fractions, or None for NaN) of one tile."""
    h = np.zeros(B, dtype=np.uint32)
    i = np.arange(B)
    if kind == "uniform":      # ny = c / (256 c) = 1/256 < 1/32: nothing clipped, clipAdd = 0, y[i] = (i + 1) / 256
        h[:] = arg
        y = [Fraction(k + 1, 256) for k in i]
    elif kind == "one":        # ny[b] = 1 -> 1/32, clipCount = 31/32, clipAdd = 31/8192 (:60-76); y[i] = (i + 1) 31/8192 + (i >= b) / 32
        b, c = arg
        h[b] = c
        y = [Fraction((k + 1) * 31, 8192) + (Fraction(1, 32) if k >= b else 0) for k in i]
    elif kind == "two":        # two bins at 1/2: each clipped by 15/32, clipAdd = (15/16) / 256 = 15/4096; y[i] = (i + 1) 15/4096 + #{b <= i} / 32
        b1, b2, c = arg
        h[b1] = h[b2] = c
        y = [Fraction((k + 1) * 15, 4096) + Fraction(int(k >= b1) + int(k >= b2), 32) for k in i]
    elif kind == "sparse":     # every fourth bin at 1/64 < 1/32: nothing clipped; y[i] = (i // 4 + 1) / 64
        h[::4] = arg
        y = [Fraction(k // 4 + 1, 64) for k in i]
    elif kind == "mixed":      # bin b holds 128 of 256 texels, the 128 even bins other than b one each (b is odd): ny[b] = 1/2 -> 1/32,
        b = arg                # clipAdd = (15/32) / 256 = 15/8192, the others stay at 1/256 + 15/8192: some bins above the limit, some below
        assert b % 2 == 1
        h[::2] = 1
        h[b] = 128
        y = [Fraction((k + 1) * 15, 8192) + Fraction(k // 2 + 1, 256) + (Fraction(1, 32) if k >= b else 0) for k in i]
    elif kind == "empty":      # count = 0: 0 / 0 = NaN; NaN > clipLimit is false, clipAdd = 0, every running sum is NaN
        y = None
    else:
        raise KeyError(kind)
    return h, y


def _check_curves(ob, grid):
    hist = np.zeros((T, T, B), dtype=np.uint32)
    want = np.zeros((T, T, B), dtype=F)
    for tx in range(T):
        for ty in range(T):
            h, y = _curve_expected(*grid[tx][ty])
            hist[tx, ty] = h
            if y is None:
                want[tx, ty] = np.nan
            else:
                assert all(v.denominator <= 8192 and 0 <= v <= 1 for v in y)   # dyadic with 13 fractional bits: every partial sum is an exact float32
                want[tx, ty] = [float(v) for v in y]
    pts = ob.k_clahe_grad_curve(hist)
    assert pts.shape == (T, T, B, 2)
    for tx in range(T):
        for ty in range(T):
            assert np.array_equal(pts[tx, ty, :, 0], _abscissae()), "abscissae of tile (%d, %d)" % (tx, ty)
            got, w = pts[tx, ty, :, 1], want[tx, ty]
            assert ((got == w) | (np.isnan(got) & np.isnan(w))).all(), "tile (%d, %d) %r: first bad ordinate %d" % (
                tx, ty, grid[tx][ty], int(np.argmax(~((got == w) | (np.isnan(got) & np.isnan(w))))))
    return pts


@pytest.mark.parametrize("count", [1, 3, 4096])
def test_curve_of_a_uniform_histogram_is_the_identity_ramp(ob, count):
    pts = _check_curves(ob, [[("uniform", count)] * T] * T)
    assert pts[2, 1, 255, 1] == 1.0 and pts[2, 1, 0, 1] == F(1 / 256)


@pytest.mark.parametrize("b", [0, 1, 100, 254, 255])
def test_curve_of_a_single_bin_spreads_its_clip_excess(ob, b):
    pts = _check_curves(ob, [[("one", (b, 7))] * T] * T)
    assert pts[0, 3, 255, 1] == 1.0                  # 256 * 31/8192 + 1/32 = 1
    assert pts[0, 3, b, 1] - (pts[0, 3, b - 1, 1] if b else 0) == F(1 / 32 + 31 / 8192)


def test_curve_of_two_bins_at_one_half_each(ob):
    pts = _check_curves(ob, [[("two", (10, 200, 5))] * T] * T)
    assert pts[1, 1, 255, 1] == 1.0                  # 256 * 15/4096 + 2/32 = 1


def test_curve_of_an_empty_tile_is_nan(ob):
    pts = _check_curves(ob, [[("empty", None)] * T] * T)
    assert np.isnan(pts[..., 1]).all()


def test_curves_of_sixteen_different_tiles_stay_in_their_own_slots(ob):
    """Every tile a different histogram, an empty one among them, none equal to its transposed partner: an offset or [ty][tx] error shows."""
    grid = [[("one", (0, 1)), ("uniform", 2), ("empty", None), ("two", (3, 4, 9))],
            [("sparse", 5), ("mixed", 77), ("one", (255, 64)), ("uniform", 1)],
            [("two", (0, 255, 1)), ("empty", None), ("mixed", 1), ("one", (128, 3))],
            [("one", (17, 1000)), ("sparse", 1), ("two", (126, 127, 2)), ("mixed", 255)]]
    for a in range(T):
        for b in range(a):
            assert grid[a][b] != grid[b][a]
    _check_curves(ob, grid)


# ---- clahe_grad_curve_apply.comp --------------------------------------------------------------------------------------------------------

def _points(ordinates):
    """points[tx][ty][i] = (x[i], ordinates[tx][ty][i])."""
    pts = np.zeros((T, T, B, 2), dtype=F)
    pts[..., 0] = _abscissae()
    pts[..., 1] = ordinates
    return pts


def _axis(v, g):
    """One axis of :45-79 in exact arithmetic: [(tile, weight)] for texel coordinate v and tile side g."""
    p = Fraction(v, g)
    base = p.numerator // p.denominator
    b = base + Fraction(1, 2)                        # :50-53
    d = p - b                                        # :55-58
    if d == 0:
        return [(base, Fraction(1))]                 # this axis takes no part in the blend (:61-63, :64-116)
    n = b + (1 if d > 0 else -1)                     # b + sign(d)
    tn = n.numerator // n.denominator                # floor: -1 for the neighbour left of tile 0, 4 right of tile 3
    tn = min(max(tn, 0), T - 1)                      # uint(-1.0) saturates to 0 (project decision), > 3 clips to 3 (:78-79)
    return [(min(base, T - 1), 1 - abs(b - p)), (tn, 1 - abs(n - p))]


_C = np.array([[(1 + T * tx + ty) / 32.0 for ty in range(T)] for tx in range(T)])   # 16 distinct dyadic constants, c[tx][ty] != c[ty][tx]


# Tile (tx, ty) has the constant curve c[tx][ty]: getY returns c for every s in [0, 1] (slope 0), so the output is the bilinear blend of the tile
# constants alone. With N / 4 a power of two every weight is dyadic and every product and sum below is an exact float32.
@pytest.mark.parametrize("side", [4, 8, 16, 32, 64])
def test_apply_blends_the_tile_constants_bilinearly(ob, side):
    g = side // T
    rng = np.random.default_rng(side)
    img = rng.random((side, side), dtype=F)
    img.flat[:3] = [0.0, 1.0, 254 / 256]
    out = ob.k_clahe_grad_curve_apply(img, _points(_C[:, :, None]))
    want = np.zeros((side, side), dtype=np.float64)
    kinds = set()
    for y in range(side):
        for x in range(side):
            ax, ay = _axis(x, g), _axis(y, g)
            kinds.add((len(ax), len(ay)))
            assert sum(w for _, w in ax) == 1 and sum(w for _, w in ay) == 1      # outer half tiles included
            want[y, x] = float(sum(wx * wy * Fraction(float(_C[tx, ty])) for tx, wx in ax for ty, wy in ay))
    assert kinds == ({(1, 1), (1, 2), (2, 1), (2, 2)} if g % 2 == 0 else {(2, 2)})   # tile centres exist only for an even tile side
    bad = np.argwhere(out != want)
    assert len(bad) == 0, "first differing texel (y, x) = %r: %r against %r" % (tuple(bad[0]), out[tuple(bad[0])], want[tuple(bad[0])])
    # the outermost half tiles see their own tile twice: corners are the corner tiles' constants
    h = g // 2
    if h:
        assert np.all(out[:h, :h] == _C[0, 0]) and np.all(out[:h, -h:] == _C[3, 0]) and np.all(out[-h:, :h] == _C[0, 3]) and np.all(out[-h:, -h:] == _C[3, 3])


def _identity_like_expected(s):
    """getY (:27-36) on y[i] = (i + 1) / 256, from the shader text. The first matching i wins:
      s == 0 (either sign): points[0].x == s                          -> y[0] = 1/256
      k/256 < s <= (k+1)/256, k < 254: segment k (it matches before points[k+1].x == s is tried), slope (1/256) / (1/256) = 1
                                                                      -> (s - k/256) + (k+1)/256, one rounding (s - k/256 is exact)
      254/256 < s <= 1: segment 254, whose right end is x[255] = 1: slope (1/256) / (2/256) = 1/2
                                                                      -> (s - 254/256) / 2 + 255/256
      s < 0, s > 1 (points[256] reads (0, 0): 1 <= s && 0 >= s never holds), NaN: no segment -> 0."""
    if np.isnan(s) or s < 0 or s > 1:
        return F(0)
    if s == 0:
        return F(1 / 256)
    S = Fraction(float(s))
    if S > Fraction(254, 256):
        return F(float((S - Fraction(254, 256)) / 2 + Fraction(255, 256)))
    k = math.ceil(S * 256) - 1
    return F(float(S - Fraction(k, 256) + Fraction(k + 1, 256)))


def _identity_like_inputs():
    ulp = lambda v, d: np.nextafter(F(v), F(d))
    vals = [F(0.0), F(-0.0), ulp(0, -1), ulp(0, 1), F(2.0 ** -127), F(2.0 ** -126), F(1.0), ulp(1, 2), ulp(1, 0), F(1.5), F(2.0), F(-0.25), F(np.nan), F(np.inf), F(-np.inf),
            F(254 / 256), F(255 / 256), ulp(254 / 256, 0), ulp(254 / 256, 1), ulp(255 / 256, 0), ulp(255 / 256, 1), F(509 / 512), F(511 / 512)]
    for k in range(B + 1):
        vals += [F(k / 256), F((k + 0.5) / 256)]
        if k:
            vals += [ulp(k / 256, 0), ulp(k / 256, 2)]
    return np.array(vals, dtype=F)


def test_identity_like_expectations_at_the_hand_worked_points():
    """The closed form above, at the values worked by hand in exact fractions."""
    e = _identity_like_expected
    assert e(F(0.0)) == F(1 / 256) and e(F(-0.0)) == F(1 / 256)
    assert e(F(1 / 256)) == F(2 / 256)               # segment 0: (1/256 - 0) + 1/256
    assert e(F(100 / 256)) == F(101 / 256)           # segment 99: 1/256 + 100/256
    assert e(F(254 / 256)) == F(255 / 256)           # segment 253: 1/256 + 254/256
    assert e(F(255 / 256)) == F(511 / 512)           # segment 254: (1/256) / 2 + 255/256
    assert e(F(1.0)) == F(1.0)                       # segment 254: (2/256) / 2 + 255/256
    assert e(F(509 / 512)) == F(255 / 256 + 1 / 1024)   # segment 254: (1/512) / 2 + 255/256
    assert e(np.nextafter(F(1), F(2))) == 0 and e(np.nextafter(F(0), F(-1))) == 0 and e(F(np.nan)) == 0 and e(F(np.inf)) == 0
    assert e(F(0.5 / 256)) == F(1.5 / 256)           # inside segment 0


def test_apply_on_tile_centres_is_get_y_of_the_identity_like_curve(ob):
    """Side 8: tile side 2, so the 16 texels with odd x and odd y sit on tile centres (x / 2 = tx + 0.5: d == 0 on both axes) and take getY of
    their own tile alone (:61-63): no blend arithmetic between the curve and the output."""
    side = 8
    pts = _points((np.arange(B) + 1) / 256.0)
    vals = _identity_like_inputs()
    assert len(vals) > 4 * B
    pad = (-len(vals)) % 16
    vals = np.concatenate([vals, np.zeros(pad, dtype=F)])
    for chunk in vals.reshape(-1, 16):
        img = np.full((side, side), 0.3, dtype=F)
        img[1::2, 1::2] = chunk.reshape(4, 4)
        out = ob.k_clahe_grad_curve_apply(img, pts)[1::2, 1::2].ravel()
        for s, got in zip(chunk, out):
            want = _identity_like_expected(s)
            assert got == want and not np.isnan(got), "s = %r (0x%08X): %r, expected %r" % (s, int(s.view(np.uint32)), got, want)
