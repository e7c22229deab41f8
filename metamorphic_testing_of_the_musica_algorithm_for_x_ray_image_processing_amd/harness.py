"""Metamorphic-testing harness for the MUSICA pipeline — the counterpart of the reference's
test/metamorphic_test/script.py, restated on numpy/scipy and driving libmusica_hip.so.

The reference perturbs each raw image (collimator shutters, translations, rotations, Gaussian and
Poisson noise), runs `maverick-standalone <raw> <bmp>` and records three similarities between the
processed altered image and the processed unaltered image: 1 - RMSE/255 (`mse_similarity`,
script.py:143-145), SSIM (:147-152) and histogram distances (:154-198), both "direct" and
"registration based" (the altered result cropped / rotated back onto the unaltered one, :442-456,
:484-508, :586-608). It only logs the numbers. This module keeps the alteration generators, their
parameter grids and the metric definitions, can drive the library in-process or through the drop-in CLI
exactly like `run_process` (:200-214), and exposes the relations as data so tests can assert them on
phantoms (the reference's raw_images/ are missing blobs).

The host restatements of the metrics live in metrics.py, the CSV and BMP writers in report.py; this module re-exports both, so
harness.<name> reaches every one of them, and keeps the grids and generators, the registration, Runner, run_study and the command line.
"""
import collections
import functools
import itertools
import math
import os
import subprocess
import types

import numpy as np
from scipy import ndimage

from . import processing as mp
from .metrics import *   # noqa: F401,F403 -- this module is the import surface: every restatement stays reachable as harness.<name>
from .metrics import _covariance_geometry, _inset, _joint_moments   # noqa: F401 -- the underscored ones the tests and probes use
from .report import *    # noqa: F401,F403

PROCESSING_MARGIN = 10  # script.py:24 == MUSICA_OUT_MARGIN

# alteration grids of the reference, for a 3072-pixel image (script.py:414, 459, 511, 562, 612, 636)
REF_IMAGE_SIZE = 3072
SHUTTERS = [200, 400, 600, 800, 1000]
TRANSLATIONS = [300, 600, 900, 1200, 1500]
ROTATIONS = [9, 18, 27, 36, 45]
GAUSS_SIGMAS = [4.0, 16.0, 64.0, 256.0, 1024.0]
POISSON_FACTORS = [0.1, 0.05, 0.025, 0.0125, 0.00625]
# not in the reference: the non-identity symmetries of the square (apply_symmetry), rows d4_<e> of a study run with `symmetries`
SYMMETRIES = (1, 2, 3, 4, 5, 6, 7)
# not in the reference: the radii of the resolution-loss rows (binomial_blur), rows blur_<r> of a study run with `blurs`
BLURS = (1, 2, 4, 8)
# not in the reference: the magnifications p / q of the scale rows (zoom), rows zoom_<p>_<q> of a study run with `zooms`: 1.05, 1.1,
# 1.25, 1.5 and 2, five strengths as every alteration of the reference's script has
ZOOMS = ((21, 20), (11, 10), (5, 4), (3, 2), (2, 1))
# not in the reference: the scatter fractions a / b of the veiling-glare rows (scatter), rows scatter_<R>_<a>_<b> of a study run with
# `scatters`: an extremity, 0.25, a chest (0.5 and 2 / 3) and an abdomen without a grid, five strengths as every alteration of the
# reference's script has. SCATTERS(n) gives them the box radius of the image size.
SCATTER_FRACTIONS = ((1, 10), (1, 4), (1, 2), (2, 3), (4, 5))


def SCATTERS(n):
    """The veils (R, a, b) of the scatter rows of a side-n image: SCATTER_FRACTIONS at R = clamp(round(127 n / 3072), 1, 127), the
    tent of sigma 104 pixels at 3072 scaled with the image."""
    r = min(max(int(round(127 * int(n) / 3072)), 1), mp.SCATTER_MAX_RADIUS)
    return tuple((r, a, b) for a, b in SCATTER_FRACTIONS)


# not in the reference: the amplitudes, in 1 / 256 pixel, of the local-deformation rows (warp), rows <family>_<a> of a study run with
# `warps`: 0.25, 1, 4, 8 and 16 pixels, five strengths as every alteration of the reference's script has. WARPS(n) gives the 25 fields.
WARP_AMPLITUDES = (64, 256, 1024, 2048, 4096)


def _div_nearest(a, b):
    """a / b for integers, b > 0, to nearest, ties away from zero."""
    q = (2 * abs(a) + b) // (2 * b)
    return q if a >= 0 else -q


def WARPS(n):
    """The 25 specs (name, field) of the warp rows of a side-n image, built in integers only, so that a name fixes the field on every
    machine. With M = processing.warp_nodes(n) nodes a side (enough for the raw plane at origin 0 and for the output plane at the
    margin), L = M - 1, u = 2i - L, v = 2j - L for node (row j, column i), w = (L^2 - u^2)(L^2 - v^2) (0 on the border), division to
    nearest with ties away from zero, and a in WARP_AMPLITUDES, the fields (dx, dy) are
        shift_<a>     (a, a)                         the sub-pixel and whole-pixel translation without a fill region
        stretch_<a>   (0, a v / L)                   a uniform stretch along y (breathing)
        shear_<a>     (a v / L, 0)                   a shear
        bulge_<a>     (a u w / L^5, a v w / L^5)     a local magnification that vanishes at the border; the peak is about 0.385 a
        twist_<a>     (-a v w / L^5, a u w / L^5)    a local rotation that vanishes at the border
    each an int16 (M, M, 2) array with every component within +-a."""
    m = mp.warp_nodes(n)
    el = m - 1
    families = (("shift", lambda a, u, v, w: (a, a)),
                ("stretch", lambda a, u, v, w: (0, _div_nearest(a * v, el))),
                ("shear", lambda a, u, v, w: (_div_nearest(a * v, el), 0)),
                ("bulge", lambda a, u, v, w: (_div_nearest(a * u * w, el ** 5), _div_nearest(a * v * w, el ** 5))),
                ("twist", lambda a, u, v, w: (_div_nearest(-a * v * w, el ** 5), _div_nearest(a * u * w, el ** 5))))
    specs = []
    for family, node in families:
        for a in WARP_AMPLITUDES:
            field = [[node(a, 2 * i - el, 2 * j - el, (el * el - (2 * i - el) ** 2) * (el * el - (2 * j - el) ** 2)) for i in range(m)] for j in range(m)]
            specs.append(("%s_%d" % (family, a), np.array(field, dtype=np.int16).reshape(m, m, 2)))
    return tuple(specs)


def _patch_grid(n, sizes, defaults, side, cap, what, item):
    """The grid detail_grid, edge_grid and grating_grid share, for a raw image of side n: G x G square patches on a square grid inside
    the output plane's footprint. With B = PROCESSING_MARGIN and m = n - 2B, `sizes` defaults to the longest prefix of `defaults` of
    length k with m // side(its last) >= k; G = min(m // (the largest side), cap) // k * k (ValueError if 0, naming the sizes as
    `what`), the cell C = m // G, and patch (i, j), i, j < G, row i first, is item(B + j C + C // 2, B + i C + C // 2,
    sizes[(i + j) % k], i G + j): the diagonal assignment puts every size G / k times in every row and every column of the grid, so
    in every band of the frame. A patch has side(size) <= C, so the patches are disjoint and lie inside [B, n - B)^2: shifted by -B
    (_output_patches) the list is valid for the output plane."""
    n, b = int(n), PROCESSING_MARGIN
    m = n - 2 * b
    if sizes is None:
        k = 0
        while k < len(defaults) and m // side(defaults[k]) >= k + 1:
            k += 1
        sizes = defaults[:k]
    sizes = tuple(int(v) for v in sizes)
    k = len(sizes)
    g = min(m // max(side(v) for v in sizes), cap) // k * k if k else 0
    if g <= 0:
        raise ValueError("a side of %d pixels holds no grid of the %s %r" % (n, what, sizes))
    c = m // g
    return [item(b + j * c + c // 2, b + i * c + c // 2, sizes[(i + j) % k], i * g + j) for i in range(g) for j in range(g)]


def _output_patches(items):
    """A raw plane's patches (x, y, ...) in the coordinates of the output plane (the frame cropped by PROCESSING_MARGIN on every side)."""
    return tuple((t[0] - PROCESSING_MARGIN, t[1] - PROCESSING_MARGIN) + tuple(t[2:]) for t in items)


# not in the reference: the contrast-detail rows (insert_details), rows cd_<c> of a study run with `details`: discs of the radii
# DETAIL_RADII on a grid (detail_grid), one row per contrast c / 1024 = 0.8 % .. 12.5 %, five strengths as every alteration of the
# reference's script has. DETAILS(n) gives the five grids of the image size.
DETAIL_RADII = (1, 2, 4, 8, 16, 32)
DETAIL_CONTRASTS = (8, 16, 32, 64, 128)


def detail_grid(n, contrast, radii=None):
    """The study's contrast-detail phantom for a raw image of side n: _patch_grid's G x G details of one contrast, their sizes the
    radii (default: a prefix of DETAIL_RADII), a box's side 4r + 5, G at most 32: detail (i, j) is (x, y, radii[(i + j) % k], contrast),
    so every radius lies G / k times in every row and every column of the grid."""
    return mp.detail_list(_patch_grid(n, radii, DETAIL_RADII, lambda r: 4 * r + 5, 32, "radii", lambda x, y, r, t: (x, y, r, contrast)), n)


def output_details(details):
    """A raw plane's details in the coordinates of the output plane (_output_patches)."""
    return _output_patches(details)


def DETAILS(n):
    """The five grids of the cd_ rows of a side-n image: detail_grid(n, c) for c in DETAIL_CONTRASTS."""
    return tuple(detail_grid(n, c) for c in DETAIL_CONTRASTS)


# not in the reference: the edge-response rows (insert_edges), rows edge_<c> of a study run with `edges`: slanted-edge plates of the
# half-sides EDGE_HALVES, the slopes EDGE_SLOPES and all four orientations on a grid (edge_grid), one row per contrast c / 1024 =
# 0.8 % .. 12.5 %, the cd_ rows' five strengths. EDGES(n) gives the five grids of the image size.
EDGE_HALVES = (8, 16, 32, 64)
# 1/8 (7.1 degrees) and 1/5 (11.3) bracket the 5 .. 10 degrees the standards ask for; 1/12 (4.8) is their lower end and 2/7 (15.9) a
# steep one with p > 1, whose bins interleave two pixel phases. Every q >= 4: every central bin is filled (edge_statistics).
EDGE_SLOPES = ((1, 8), (1, 5), (1, 12), (2, 7))
EDGE_CONTRASTS = (8, 16, 32, 64, 128)


def edge_grid(n, contrast, halves=None):
    """The study's edge phantom for a raw image of side n: _patch_grid's G x G plates of one contrast, their sizes the half-sides
    (default: a prefix of EDGE_HALVES), a plate's side 4h + 1, G at most 16 (256 = EDGE_MAX plates): edge t = i G + j is (x, y,
    halves[(i + j) % k], *EDGE_SLOPES[(t // 4) % 4], t % 4, contrast), so every half-side lies G / k times in every row and every
    column of the grid, the orientations cycle fastest and the slopes behind them."""
    return mp.edge_list(_patch_grid(n, halves, EDGE_HALVES, lambda h: 4 * h + 1, 16, "half-sides",
                                    lambda x, y, h, t: (x, y, h) + EDGE_SLOPES[(t // 4) % len(EDGE_SLOPES)] + (t % 4, contrast)), n)


def output_edges(edges):
    """A raw plane's edges in the coordinates of the output plane (_output_patches)."""
    return _output_patches(edges)


def EDGES(n):
    """The five grids of the edge_ rows of a side-n image: edge_grid(n, c) for c in EDGE_CONTRASTS."""
    return tuple(edge_grid(n, c) for c in EDGE_CONTRASTS)


# not in the reference: the grating rows (insert_gratings), rows grating_<c> of a study run with `gratings`: cosine patches of the periods
# GRATING_PERIODS in the directions GRATING_DIRECTIONS on a grid (grating_grid), one row per contrast c / 1024 = 0.8 % .. 12.5 %, the
# cd_ and edge_ rows' five strengths. GRATINGS(n) gives the five grids of the image size.
# 0.5 cycles / pixel (the pixel grid's Nyquist frequency along an axis) down to 1 / 32, two steps an octave from T = 2: the band a
# multi-scale processor's finer levels divide between them. Along the diagonals the frequency is sqrt(2) / T.
GRATING_PERIODS = (2, 3, 4, 6, 8, 12, 16, 24, 32)
GRATING_DIRECTIONS = ((1, 0), (0, 1), (1, 1), (1, -1))
GRATING_CONTRASTS = (8, 16, 32, 64, 128)


def grating_half(period):
    """The half-side of the phantom's plate of a period: max(8, 2T), so the measured region holds at least four periods."""
    return max(mp.GRATING_MIN_HALF, 2 * int(period))


def grating_grid(n, contrast, periods=None):
    """The study's grating phantom for a raw image of side n: _patch_grid's G x G plates of one contrast, their sizes the periods
    (default: a prefix of GRATING_PERIODS), a plate's side 4 h(T) + 1 with h(T) = grating_half(T), G at most 16 (256 = GRATING_MAX
    plates): grating t = i G + j is (x, y, h(T), *GRATING_DIRECTIONS[t % 4], T, grating_wave(T, contrast)) with T = periods[(i + j) % k],
    so every period lies G / k times in every row and every column of the grid, the directions cycle fastest. (Which directions a
    period meets depends on G mod 4: for G = 9, t = i + j mod 4, so a period meets two neighbouring directions; the "directions"
    groups and "per_grating" keep them apart.)"""
    return mp.grating_list(_patch_grid(n, periods, GRATING_PERIODS, lambda t: 4 * grating_half(t) + 1, 16, "periods",
                                       lambda x, y, p, t: (x, y, grating_half(p)) + GRATING_DIRECTIONS[t % len(GRATING_DIRECTIONS)] + (p, grating_wave(p, contrast))), n)


def output_gratings(gratings):
    """A raw plane's gratings in the coordinates of the output plane (_output_patches)."""
    return _output_patches(gratings)


def GRATINGS(n):
    """The five grids of the grating_ rows of a side-n image: grating_grid(n, c) for c in GRATING_CONTRASTS."""
    return tuple(grating_grid(n, c) for c in GRATING_CONTRASTS)


def grating_contrast(gratings):
    """The contrast a grating list is named after: the largest |w| of its first grating's wave (grating_wave(T, c): |c|)."""
    return max(abs(w) for w in gratings[0][6])


# not in the reference: the point-response rows (insert_points), rows point_<c> of a study run with `points`: defect pixels and 2 x 2
# and 3 x 3 clusters on a grid (point_grid), each with a window of half-side POINT_RADIUS around it, one row per contrast c / 1024: a
# dead element, a half-dead and a faint one, a doubled and a hot one. POINTS(n) gives the five grids of the image size.
POINT_RADIUS = 16
POINT_SIZES = (1, 2, 3)
POINT_CONTRASTS = (1024, 512, 64, -1024, -64512)


def point_grid(n, contrast, sizes=None, radius=POINT_RADIUS):
    """The study's point phantom for a raw image of side n: _patch_grid's G x G points of one contrast and one window half-side, their
    sizes the cluster sizes (default: a prefix of POINT_SIZES), a window's side 2 radius + 1, G at most 64 (63 x 63 = 3969 <= POINT_MAX
    points at n = 3072): point (i, j) is (x, y, radius, sizes[(i + j) % k], contrast, (i + j) % k), so every size lies G / k times in
    every row and every column of the grid and the group is the index of the size."""
    order = POINT_SIZES if sizes is None else tuple(int(v) for v in sizes)
    return mp.point_list(_patch_grid(n, sizes, POINT_SIZES, lambda s: 2 * int(radius) + 1, 64, "cluster sizes",
                                     lambda x, y, s, t: (x, y, int(radius), s, contrast, order.index(s))), n)


def output_points(points):
    """A raw plane's points in the coordinates of the output plane (_output_patches)."""
    return _output_patches(points)


def POINTS(n):
    """The five grids of the point_ rows of a side-n image: point_grid(n, c) for c in POINT_CONTRASTS."""
    return tuple(point_grid(n, c) for c in POINT_CONTRASTS)


# not in the reference: the detector-gain rows (apply_gain), rows named by the spec of a study run with `gains`: a separable gain map
# out = v gx[x] gy[y] in units of 1 / 4096 (processing.GAIN_ONE), scored like every row and by the exact row and column profiles of the
# result against the unaltered result (profile_statistics). A spec is (name, gx, gy); GAINS(n) gives the 25 of the image size: the
# exposures GAIN_EXPOSURES, and for each strength c of GAIN_CONTRASTS (c / 1024 = 0.8 % .. 12.5 %, the cd_, edge_ and grating_ rows' five)
# a heel effect, a vignetting, gain bands and defective lines. Every builder works on Python ints.
GAIN_EXPOSURES = ((1, 4), (1, 2), (3, 4), (3, 2), (2, 1))
GAIN_CONTRASTS = (8, 16, 32, 64, 128)


def _gain_side(n):
    n = int(n)
    if n < 2:
        raise ValueError("a gain map needs a side of at least 2, got %d" % n)
    return n


def gain_exposure(n, num, den):
    """The dose changed by num / den: gx[i] = 4096, gy[i] = (4096 num + den // 2) // den (the ratio rounded to 1 / 4096, halves up), the
    same for every i: every pixel is multiplied by one constant."""
    n, num, den = _gain_side(n), int(num), int(den)
    g = (mp.GAIN_ONE * num + den // 2) // den
    if num < 0 or den < 1 or g > 65535:
        raise ValueError("exposure %d / %d is not a gain of 0 .. 65535 / 4096" % (num, den))
    return [mp.GAIN_ONE] * n, [g] * n


def gain_heel(n, c):
    """The heel effect, a linear ramp down the rows of c / 1024 peak to peak: with m = n - 1 and t = 2 i - m (-m .. m),
    gy[i] = 4096 + (4 c t + m) // (2 m) (2 c t / m rounded, halves up: -2c at the top row, +2c at the bottom), gx[i] = 4096."""
    n, c = _gain_side(n), int(c)
    m = n - 1
    return [mp.GAIN_ONE] * n, [mp.GAIN_ONE + (4 * c * (2 * i - m) + m) // (2 * m) for i in range(n)]


def gain_vignette(n, c):
    """Vignetting, a separable parabola that is c / 1024 down at the corners: with m = n - 1 and t = 2 i - m,
    gx[i] = gy[i] = 4096 - (2 c t^2 + m^2 // 2) // m^2 (2 c (t / m)^2 rounded, halves up: 0 at the centre, 2c down at either end of an
    axis, so 4c / 4096 = c / 1024 down where both ends meet)."""
    n, c = _gain_side(n), int(c)
    m = n - 1
    g = [mp.GAIN_ONE - (2 * c * (2 * i - m) ** 2 + m * m // 2) // (m * m) for i in range(n)]
    return g, list(g)


def gain_bands(n, c):
    """Gain bands, readout blocks whose calibration is off: blocks of B = max(16, n // 16) columns alternate between 4096 + 2c (the
    first) and 4096 - 2c, gx[i] = 4096 + 2c if (i // B) % 2 == 0 else 4096 - 2c, gy[i] = 4096: every block border is a step of
    4c / 4096 = c / 1024."""
    n, c = _gain_side(n), int(c)
    b = max(16, n // 16)
    return [mp.GAIN_ONE + 2 * c if (i // b) % 2 == 0 else mp.GAIN_ONE - 2 * c for i in range(n)], [mp.GAIN_ONE] * n


def gain_line_positions(n):
    """Where gain_lines puts its nine lines along an axis: PROCESSING_MARGIN + (2 j + 1) (n - 20) // 18 for j = 0 .. 8, the centres of
    nine equal parts of the output plane's footprint; inside it for n >= 84."""
    n = _gain_side(n)
    return [PROCESSING_MARGIN + (2 * j + 1) * (n - 2 * PROCESSING_MARGIN) // 18 for j in range(9)]


def gain_lines(n, c):
    """Defective lines: the nine columns and the nine rows at gain_line_positions(n) have the gain 4096 - 4c (c / 1024 down), every
    other line 4096. A crossing is down by both."""
    n, c = _gain_side(n), int(c)
    at = set(gain_line_positions(n))
    if not all(0 <= p < n for p in at):
        raise ValueError("a side of %d pixels does not hold the nine lines" % n)
    g = [mp.GAIN_ONE - 4 * c if i in at else mp.GAIN_ONE for i in range(n)]
    return g, list(g)


def GAINS(n):
    """The 25 gain specs (name, gx, gy) of a side-n image: exposure_<num>_<den> for GAIN_EXPOSURES, then heel_<c>, vignette_<c>,
    band_<c> and line_<c>, each for c in GAIN_CONTRASTS."""
    out = [("exposure_%d_%d" % e,) + gain_exposure(n, *e) for e in GAIN_EXPOSURES]
    for name, build in (("heel", gain_heel), ("vignette", gain_vignette), ("band", gain_bands), ("line", gain_lines)):
        out += [("%s_%d" % (name, c),) + build(n, c) for c in GAIN_CONTRASTS]
    return tuple(out)


def output_gain(spec):
    """A raw plane's gain spec (name, gx, gy) in the coordinates of the output plane (the frame cropped by PROCESSING_MARGIN on every
    side): (gx, gy) sliced."""
    _, gx, gy = spec
    return tuple(gx[PROCESSING_MARGIN:len(gx) - PROCESSING_MARGIN]), tuple(gy[PROCESSING_MARGIN:len(gy) - PROCESSING_MARGIN])


def apply_gain(image, gx, gy):
    """The square 2-D uint16 plane under the separable gain map (processing.gain_tables for its side, else ValueError before any work):
        g   = gx[x] * gy[y]                              (fits uint32)
        out = min((v * g + 2^23) >> 24, 65535)           ONE rounding, halves up, in uint64: the largest intermediate is 65535^3 + 2^23 < 2^48
    gx = gy = 4096 returns v exactly; the clamp is the detector's saturation."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype != np.uint16 or not image.size:
        raise ValueError("apply_gain needs a non-empty square 2-D uint16 plane, got %r %s" % (image.shape, image.dtype))
    gx, gy = mp.gain_tables(gx, gy, image.shape[0])
    g = gx.astype(np.uint64)[None, :] * gy.astype(np.uint64)[:, None]
    return np.minimum((image.astype(np.uint64) * g + np.uint64(1 << 23)) >> np.uint64(24), np.uint64(65535)).astype(np.uint16)


# not in the reference: the tone-table rows (apply_lut), rows named by the spec of a study run with `luts`: the raw image mapped point-wise
# through a 65536-entry table, out = lut[v], scored like every row and by the exact sums of the result against the unaltered result per
# level of the unaltered INPUT (level_statistics): the chain's characteristic curve before and after. A spec is (name, lut); LUTS(raw)
# gives the 21 of a raw plane, built from its own range: a pedestal, saturation, a coarser ADC, a non-linear characteristic, a negative.
LUT_CONTRASTS = (8, 16, 32, 64, 128)
LUT_BITS = (12, 10, 8, 7, 6)
LUT_GAMMAS = ((3, 4), (9, 10), (11, 10), (5, 4), (3, 2))


def LUTS(raw):
    """The 21 tone-table specs (name, lut) of a raw plane, each lut a uint16 array of 65536 entries, from the plane's own range lo =
    min, hi = max, span = hi - lo (ValueError if span < 1024); v runs over 0 .. 65535 and c over LUT_CONTRASTS:
        offset_<c>          min(v + ((c span + 512) >> 10), 65535): a dark-current pedestal of c / 1024 of the span
        clip_<c>            min(v, hi - ((c span) >> 10)): saturation of the top c / 1024 of the span
        bits_<b>            v & ~((1 << s) - 1) with s = max(0, span.bit_length() - b), b in LUT_BITS: an ADC that leaves about b bits
                            of the span
        gamma_<num>_<den>   lo + rint(span ((v - lo) / span)^(num / den)) on lo <= v <= hi, v outside, (num, den) in LUT_GAMMAS: a
                            non-linear characteristic that keeps both ends of the range (f64 pow, here, once: the table is the payload)
        negative            lo + hi - v on lo <= v <= hi, v outside
    Every table but `negative` is non-decreasing."""
    raw = np.asarray(raw)
    if raw.dtype != np.uint16 or not raw.size:
        raise ValueError("LUTS needs a non-empty uint16 plane, got %r %s" % (raw.shape, raw.dtype))
    lo, hi = int(raw.min()), int(raw.max())
    span = hi - lo
    if span < 1024:
        raise ValueError("the plane's range %d .. %d spans less than 1024 levels" % (lo, hi))
    v = np.arange(mp.LUT_ENTRIES, dtype=np.int64)
    inside = (v >= lo) & (v <= hi)
    out = [("offset_%d" % c, np.minimum(v + ((c * span + 512) >> 10), 65535)) for c in LUT_CONTRASTS]
    out += [("clip_%d" % c, np.minimum(v, hi - ((c * span) >> 10))) for c in LUT_CONTRASTS]
    out += [("bits_%d" % b, v & ~((1 << max(0, span.bit_length() - b)) - 1)) for b in LUT_BITS]
    unit = np.clip((v - lo) / span, 0.0, 1.0)
    out += [("gamma_%d_%d" % (num, den), np.where(inside, lo + np.rint(span * np.power(unit, num / den)).astype(np.int64), v)) for num, den in LUT_GAMMAS]
    out.append(("negative", np.where(inside, lo + hi - v, v)))
    return tuple((name, lut.astype(np.uint16)) for name, lut in out)


def apply_lut(image, lut):
    """The square 2-D uint16 plane mapped point-wise through the tone table (processing.lut_table: 65536 integers in 0 .. 65535, else
    ValueError before any work): lut[image]. lut = arange(65536) copies the image. This is the contract of musica_alter_lut
    (include/musica.h), which is bit-identical to it."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype != np.uint16 or not image.size:
        raise ValueError("apply_lut needs a non-empty square 2-D uint16 plane, got %r %s" % (image.shape, image.dtype))
    return mp.lut_table(lut)[image]


def level_shift(raw):
    """The shift of a study's classes: the smallest that puts raw.max() below 4096 classes, and never less than LEVEL_MIN_SHIFT = 4."""
    return max(mp.LEVEL_MIN_SHIFT, int(np.asarray(raw).max()).bit_length() - 12)


def level_classes(raw, shift):
    """The class plane of the output of a square 2-D uint16 raw plane: raw[M:-M, M:-M] >> shift with M = PROCESSING_MARGIN, the level of
    the unaltered input under every output pixel; shift an integer 4 .. 15 (processing.level_count: (65535 >> shift) + 1 <= 4096
    classes), else ValueError."""
    mp.level_count(shift)
    raw = np.asarray(raw)
    if raw.ndim != 2 or raw.shape[0] != raw.shape[1] or raw.dtype != np.uint16 or raw.shape[0] <= 2 * PROCESSING_MARGIN:
        raise ValueError("level_classes needs a square 2-D uint16 plane of a side above %d, got %r %s" % (2 * PROCESSING_MARGIN, raw.shape, raw.dtype))
    return raw[PROCESSING_MARGIN:-PROCESSING_MARGIN, PROCESSING_MARGIN:-PROCESSING_MARGIN] >> np.uint16(shift)


def REACH_RADII(n):
    """The default radii of a study's reach classes for a raw plane of side n: 0, then the half-octaves 1, 2, 3, 4, 6, 8, 12, 16, 24, ..
    (2^k and 3 * 2^(k - 1)) up to the largest below n; at most REACH_MAX_RADII = 32 entries (28 at the largest side, 16384)."""
    radii, k = [0], 0
    while True:
        for r in ((1 << k),) + ((3 << (k - 1),) if k >= 1 else ()):
            if r >= n or len(radii) == mp.REACH_MAX_RADII:
                return radii
            radii.append(r)
        k += 1


def scaled(values, image_size):
    """The reference's pixel-valued grids scaled from 3072 to `image_size`."""
    return [max(1, int(round(v * image_size / REF_IMAGE_SIZE))) for v in values]


# ---- alteration generators (script.py:49-141) ------------------------------------------------------

def apply_quantum_noise(image, scale_factor=1.0, rng=None):
    """script.py:49-58: Poisson noise at `scale_factor` of the dose."""
    rng = rng or np.random.default_rng()
    scaled_image = image.astype(np.float64) * scale_factor
    noisy = rng.poisson(scaled_image).astype(np.float32) / scale_factor
    return np.clip(noisy, 0, 65535).astype(np.uint16)


def add_gaussian_noise(image, mean, sigma, rng=None):
    """script.py:60-66: additive Gaussian noise, truncated to int before the add."""
    rng = rng or np.random.default_rng()
    noise = rng.normal(mean, sigma, image.shape).astype(np.int32)
    return np.clip(image.astype(np.int32) + noise, 0, 65535).astype(np.uint16)


def apply_collimator(image, shutter_h, shutter_v, rng=None):
    """script.py:75-95: outside the shutter rectangle the detector sees 1 % of the dose (+ Poisson noise)."""
    h, w = image.shape
    mask = np.zeros((h, w), dtype=bool)
    mask[shutter_v:h - shutter_v + 1, shutter_h:w - shutter_h + 1] = True   # PIL rectangles include both corners
    low = apply_quantum_noise((image / 100).astype(np.float64), 1, rng)
    return np.where(mask, image, low).astype(np.uint16)


def clamp_translation(image, x_shift, y_shift=0):
    """script.py:97-120: shift, filling the uncovered band with the 99th percentile of a 2-pixel strip."""
    h, w = image.shape
    bright, margin = 2, 10
    left = margin if x_shift > 0 else 0
    right = w - margin if x_shift < 0 else w
    top = margin if y_shift > 0 else 0
    bottom = h - margin if y_shift < 0 else h
    cropped = image[top:bottom, left:right]
    b_right = margin + bright if x_shift > 0 else w
    b_bottom = margin + bright if y_shift > 0 else h
    fill = int(np.percentile(image[top:b_bottom, left:b_right], 99))
    out = np.full((h, w), fill, dtype=np.uint16)
    ys, xs = max(y_shift, 0), max(x_shift, 0)
    hh, ww = min(cropped.shape[0], h - ys), min(cropped.shape[1], w - xs)
    out[ys:ys + hh, xs:xs + ww] = cropped[:hh, :ww]
    return out


def clamp_rotate(image, degree):
    """script.py:122-141: rotate the image minus a 100-pixel margin (nearest neighbour, counter-clockwise),
    filling with the 95th percentile."""
    h, w = image.shape
    margin = min(100, h // 8)
    cropped = image[margin:h - margin, margin:w - margin]
    fill = int(np.percentile(cropped, 95))
    rot = ndimage.rotate(cropped, degree, reshape=False, order=0, mode="constant", cval=fill)
    out = np.full((h, w), fill, dtype=np.uint16)
    out[margin:h - margin, margin:w - margin] = rot
    return out


def apply_symmetry(image, element):
    """Element 0 .. 7 of the symmetry group of the square (D4): np.rot90(x if element < 4 else x.T, element & 3). Output pixel (i, j) of
    a side-n plane is input pixel 0: [i, j], 1: [j, n-1-i], 2: [n-1-i, n-1-j], 3: [n-1-j, i], 4: [j, i] (transpose), 5: [n-1-i, j]
    (flipud), 6: [n-1-j, n-1-i] (anti-transpose), 7: [i, n-1-j] (fliplr): a permutation of the pixels, no fill and no resampling
    (not in the reference's script). Inverses: 1 <-> 3, every other element is its own."""
    element = int(element)
    if not 0 <= element <= 7:
        raise ValueError("symmetry element %d is not in 0 .. 7" % element)
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1]:
        raise ValueError("the symmetries of the square need a square image, got %r" % (image.shape,))
    return np.ascontiguousarray(np.rot90(image if element < 4 else image.T, element & 3))


def binomial_blur(image, radius):
    """The exact binomial blur of a 2-D uint16 or uint8 plane (not in the reference's script): resolution loss in integers. With
    r = radius in 1 .. BLUR_MAX_RADIUS and the weights w_k = C(2r, k), k = 0 .. 2r (their sum is 4^r),
        out[y, x] = (sum_i sum_j w_i w_j in[clamp(y + i - r), clamp(x + j - r)] + 2^(4r - 1)) >> 4r
    with indices clamped to the plane (edge replicated, no fill value). ONE rounding, after the full 2-D sum, halves rounded up; nothing
    is rounded between the two passes. The result has the input's dtype; a constant plane is preserved, so nothing saturates. The largest
    radius follows from the widths: the row pass of u16 data needs 16 + 2r <= 32 bits, the full sum 16 + 4r <= 48 (u64 here). At r = 8
    the blur is a Gaussian of sigma = sqrt(r / 2) = 2 pixels. This is the contract of musica_alter_blur and musica_sim_blur_reference
    (include/musica.h), which are bit-identical to it."""
    r = int(radius)
    if not 1 <= r <= mp.BLUR_MAX_RADIUS:
        raise ValueError("blur radius %d is not in 1 .. %d" % (r, mp.BLUR_MAX_RADIUS))
    image = np.asarray(image)
    if image.ndim != 2 or image.dtype not in (np.uint16, np.uint8) or not image.size:
        raise ValueError("binomial_blur needs a non-empty 2-D uint16 or uint8 plane, got %r %s" % (image.shape, image.dtype))
    acc = image.astype(np.uint64)
    for axis in (1, 0):           # rows, then columns: exact integers, so the order changes nothing
        padded = np.pad(acc, [(r, r) if a == axis else (0, 0) for a in (0, 1)], mode="edge")   # the clamped indices
        acc = np.zeros_like(acc)
        for k in range(2 * r + 1):
            acc += np.uint64(math.comb(2 * r, k)) * (padded[k:k + acc.shape[0]] if axis == 0 else padded[:, k:k + acc.shape[1]])
    return ((acc + np.uint64(1 << (4 * r - 1))) >> np.uint64(4 * r)).astype(image.dtype)


def zoom(image, ratio):
    """The exact rational zoom of a square 2-D uint16 or uint8 plane of side n (not in the reference's script): magnification by p / q
    about the plane's centre, bilinear, in integers. ratio = (p, q), integers 1 <= q < p <= ZOOM_MAX_P = 32 with gcd(p, q) = 1, else
    ValueError before any work. With D = 2p, for an output index x
        n_x = (2x - (n - 1)) q + (n - 1) p        (>= 0; the source coordinate is n_x / D = (x - c) q / p + c, c = (n - 1) / 2)
        i_x = n_x div D,   f_x = n_x mod D,   g_x = D - f_x,   i+ = min(i + 1, n - 1)
        out[y, x] = (g_y g_x in[i_y, i_x] + g_y f_x in[i_y, i_x+] + f_y g_x in[i_y+, i_x] + f_y f_x in[i_y+, i_x+] + D^2 / 2) div D^2
    ONE rounding, after the full 2-D sum, halves rounded up. The result has the input's dtype. The weights sum to D^2 <= 4096 and the
    sum is at most 65535 * 4096 + 2048 < 2^32: every intermediate fits u32, and a constant plane is preserved. A zoom above 1 about the
    centre reads only inside the plane, so there is no fill value: i_x <= n - 2 everywhere except where f_x = 0, and there the clamped
    neighbour's weight is 0. Mirroring x -> n - 1 - x maps n_x -> 2p (n - 1) - n_x, so the map commutes exactly with all eight
    apply_symmetry elements. And 2 (x + 10) - (N - 1) = 2x - (M - 1) for M = N - 20: the zoom of the output plane (the full frame
    cropped by PROCESSING_MARGIN on every side) is the crop of the zoom of the full frame, which is what makes register_zoom meaningful.
    This is the contract of musica_alter_zoom and musica_sim_zoom_reference (include/musica.h), which are bit-identical to it."""
    p, q = mp.zoom_ratio(ratio)
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype not in (np.uint16, np.uint8) or not image.size:
        raise ValueError("zoom needs a non-empty square 2-D uint16 or uint8 plane, got %r %s" % (image.shape, image.dtype))
    n, d = image.shape[0], 2 * p
    num = (2 * np.arange(n, dtype=np.int64) - (n - 1)) * q + (n - 1) * p
    i, f = num // d, (num % d).astype(np.uint64)
    g, i1 = np.uint64(d) - f, np.minimum(i + 1, n - 1)
    a = image.astype(np.uint64)
    top, bottom = (a[r][:, i] * g + a[r][:, i1] * f for r in (i, i1))       # the rows i_y and i_y+, folded along x
    return ((g[:, None] * top + f[:, None] * bottom + np.uint64(d * d // 2)) // np.uint64(d * d)).astype(image.dtype)


def warp(image, field, origin=(0, 0)):
    """The exact grid warp of a square 2-D uint16 or uint8 plane of side n (not in the reference's script): a local deformation, the
    backward warp out[x] = in[x + d(x)] (no holes, no folds) by a displacement field on a control grid of spacing G = 64 pixels. field
    is an (M, M, 2) array of integers, field[j, i] = (dx, dy) at node (row j, column i) in units of 1 / 256 pixel, every component within
    +-WARP_MAX_SHIFT = 4096 (16 pixels). origin = (ox, oy), 0 <= ox, oy < 64: pixel (x, y) of this plane sits at grid coordinate
    (x + ox, y + oy); M >= ((n - 1 + max(ox, oy)) >> 6) + 2 and nodes beyond that count are ignored, so one node array serves the raw
    plane (origin 0) and the output plane cropped by PROCESSING_MARGIN (origin 10). ValueError before any work otherwise
    (processing.warp_field). Everything is integer arithmetic, `>>` the arithmetic shift (a floor). For output pixel (x, y):
        X = x + ox,  cx = X >> 6,  fx = X & 63                                     (Y, cy, fy likewise from y + oy)
        per component c (0: dx, 1: dy), d = field[.., .., c]:
          S_c = (64 - fy) ((64 - fx) d[cy, cx]     + fx d[cy, cx + 1])
              +       fy  ((64 - fx) d[cy + 1, cx] + fx d[cy + 1, cx + 1])         |S_c| <= 2^24
          s_c = (S_c + 2048) >> 12                                                 1 / 256 px; |s_c| <= max |d| (convex weights, one rounding)
        ix = x + (s_0 >> 8),  wx = s_0 & 255                                       (iy, wy likewise from s_1)
        x0 = clamp(ix), x1 = clamp(ix + 1), y0 = clamp(iy), y1 = clamp(iy + 1)     clamp to 0 .. n - 1: edge replicated, no fill value
        out[y, x] = ((256 - wy) ((256 - wx) in[y0, x0] + wx in[y0, x1]) + wy ((256 - wx) in[y1, x0] + wx in[y1, x1]) + 32768) >> 16
    ONE rounding of the field and ONE of the image sum, halves up; nothing is rounded between the two image passes. The sum is at most
    65535 * 65536 + 32768 < 2^32: every intermediate fits i32 or u32. The result has the input's dtype. The sign agrees with
    displacement_table: an output that follows the input has its best shift at +d.
      * The zero field is the identity.
      * A constant field of whole pixels (256 kx, 256 ky) is in[clamp(y + ky), clamp(x + kx)] exactly; a constant field survives the
        interpolation unchanged because (4096 d + 2048) >> 12 = d.
      * A constant plane is preserved for every field: the weights are convex, nothing saturates.
      * Reach: warp_reach(field) = (max |d| + 255) // 256 + 1, and a pixel reads only within the reach of itself.
      * Cropping commutes inside the reach: warp(P, F)[10:-10, 10:-10] and warp(P[10:-10, 10:-10], F, origin=(10, 10)) agree
        everywhere except within warp_reach(F) of the border, where they do differ because the cropped plane clamps: the registered
        region is inset by the reach (register_warp, roi_warp).
      * No commutation with the apply_symmetry elements is claimed: the floors are not mirror-symmetric.
    This is the contract of musica_alter_warp and musica_sim_warp_reference (include/musica.h), which take one origin for both axes and
    are bit-identical to it."""
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype not in (np.uint16, np.uint8) or not image.size:
        raise ValueError("warp needs a non-empty square 2-D uint16 or uint8 plane, got %r %s" % (image.shape, image.dtype))
    try:
        ox, oy = origin
    except (TypeError, ValueError):
        raise ValueError("an origin is a pair (ox, oy), got %r" % (origin,))
    n = image.shape[0]
    for o in (ox, oy):
        field = mp.warp_field(field, n, o)
    s0, s1 = warp_shifts(field, np.arange(n) + int(ox), np.arange(n) + int(oy))
    ix, iy = np.arange(n)[None, :] + (s0 >> 8), np.arange(n)[:, None] + (s1 >> 8)
    wx, wy = (s0 & 255).astype(np.uint64), (s1 & 255).astype(np.uint64)
    x0, x1, y0, y1 = (np.clip(v, 0, n - 1) for v in (ix, ix + 1, iy, iy + 1))
    a, one = image.astype(np.uint64), np.uint64(256)
    top = (one - wx) * a[y0, x0] + wx * a[y0, x1]
    bottom = (one - wx) * a[y1, x0] + wx * a[y1, x1]
    return (((one - wy) * top + wy * bottom + np.uint64(32768)) >> np.uint64(16)).astype(image.dtype)


def warp_reach(field):
    """(max |d| + 255) // 256 + 1: how far, in pixels, warp reads from an output pixel at most (the whole pixels of the largest
    displacement, rounded up, and the bilinear neighbour)."""
    return (int(np.abs(np.asarray(field).astype(np.int64)).max()) + 255) // 256 + 1


def _box(acc, radius, axis):
    """sum_{k = -R .. R} acc[clamp(i + k)] along `axis` of a uint64 array: np.pad(mode="edge"), then the (2R + 1)-window sum as the
    difference of two entries of the padded array's cumulative sum."""
    r = int(radius)
    padded = np.pad(acc, [(r, r) if a == axis else (0, 0) for a in (0, 1)], mode="edge")   # the clamped indices
    total = np.cumsum(padded, axis=axis, dtype=np.uint64)
    total = np.concatenate([np.zeros_like(total[:1] if axis == 0 else total[:, :1]), total], axis=axis)
    n = acc.shape[axis]
    if axis == 0:
        return total[2 * r + 1:2 * r + 1 + n] - total[:n]
    return total[:, 2 * r + 1:2 * r + 1 + n] - total[:, :n]


def scatter(image, spec):
    """The exact wide veiling glare of a square 2-D uint16 or uint8 plane (not in the reference's script): scattered radiation under
    automatic exposure control, a very wide, smooth veil that displaces primary signal at the scatter fraction SF = S / (S + P) = a / b.
    spec = (R, a, b): the box radius 1 <= R <= SCATTER_MAX_RADIUS = 127 and integers 1 <= a < b <= SCATTER_MAX_DEN = 64 with
    gcd(a, b) = 1, else ValueError before any work. With box_axis(A)[i] = sum_{k = -R .. R} A[clamp(i + k)], clamped to the plane (edge
    replicated; each pass clamps its own input: np.pad(mode="edge") and a (2R + 1)-window sum), in uint64
        V   = box_y(box_y(box_x(box_x(image))))          tent x tent, total weight W = (2R + 1)^4
        out = ((b - a) W image + a V + (b W) // 2) // (b W)
    ONE rounding, after the full sum, halves rounded up; nothing is rounded between the passes. The result has the input's dtype.
      * The row and column operators commute: the order of the four passes changes nothing.
      * After the two row passes a value is at most 255^2 * 65535 = 4 261 413 375 < 2^32 (the device's row-pass plane is u32).
      * W <= 255^4 = 4 228 250 625 < 2^32.
      * The full numerator is at most 65535 * 64 * 255^4, about 1.77e16 < 2^64: the column passes and the mix are u64. The cumulative
        sums here stay below 255^3 * 65535 * (16384 + 254) < 2^64 for every side a context accepts.
      * The weights are a convex combination: a constant plane is preserved, nothing saturates and nothing is clipped.
      * The operator commutes exactly with all eight apply_symmetry elements.
      * It does NOT commute with cropping, because the borders are clamped: within 2R pixels of the output plane's border the veiled
        reference is built from clamped neighbours, so the registered region is inset by 2R (register_scatter, roi_scatter).
      * The tent has sigma = sqrt(2R (R + 1) / 3) pixels: 104 at R = 127.
    This is the contract of musica_alter_scatter and musica_sim_scatter_reference (include/musica.h), which are bit-identical to it."""
    r, a, b = mp.scatter_spec(spec)
    image = np.asarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.dtype not in (np.uint16, np.uint8) or not image.size:
        raise ValueError("scatter needs a non-empty square 2-D uint16 or uint8 plane, got %r %s" % (image.shape, image.dtype))
    primary = image.astype(np.uint64)
    veil = primary
    for axis in (1, 1, 0, 0):     # rows twice, then columns twice: exact integers, so the order changes nothing
        veil = _box(veil, r, axis)
    w = (2 * r + 1) ** 4
    return ((np.uint64((b - a) * w) * primary + np.uint64(a) * veil + np.uint64(b * w // 2)) // np.uint64(b * w)).astype(image.dtype)


# ---- the vendor-processed reference image (script.py:395-411) ------------------------------------------

def vendor_to_u8(pixels):
    """The 8-bit image the reference compares against, from the vendor image's stored values (dicom.read_dicom_gray): for 16-bit data
    Image.point(i * 1/256).convert('L') truncates to v >> 8, and ImageOps.invert is 255 - v, whatever the DICOM's
    PhotometricInterpretation says. So 255 - (v >> 8) for uint16, 255 - v for uint8 (checked against Pillow for every value)."""
    a = np.asarray(pixels)
    if a.dtype == np.uint16:
        return (255 - (a >> 8)).astype(np.uint8)
    if a.dtype == np.uint8:
        return 255 - a
    raise ValueError("vendor image must be uint8 or uint16, got %s" % a.dtype)


# ---- registration of the altered result onto the unaltered one (script.py:442-456, 484-508, 586-608) ----
# The geometry lives in the *_rects functions: one rectangle (x, y, w, h) per side, exactly what the reference's slices select (Python's
# clamping of slice bounds included). register_* slice with them; roi_* state them as the (ax, ay, bx, by, w, h) region of a device-side
# comparison (musica_sim_compare), or None when the two slices differ in shape (the study then has no registered comparison).

def _span(start, stop, n):
    """What a[start:stop] selects along an axis of length n: (first index, length)."""
    first, end, _ = slice(start, stop).indices(n)
    return first, max(0, end - first)


def _rect(shape, y0, y1, x0, x1):
    y, h = _span(y0, y1, shape[0])
    x, w = _span(x0, x1, shape[1])
    return x, y, w, h


def _crop(alt, unalt, rects):
    (ax, ay, aw, ah), (bx, by, bw, bh) = rects
    return alt[ay:ay + ah, ax:ax + aw], unalt[by:by + bh, bx:bx + bw]


def _roi(rects):
    (ax, ay, aw, ah), (bx, by, bw, bh) = rects
    return (ax, ay, bx, by, aw, ah) if (aw, ah) == (bw, bh) else None


def collimator_rects(a_shape, b_shape, shutter):
    x = y = shutter + PROCESSING_MARGIN
    w = a_shape[1] - (2 * shutter + 2 * PROCESSING_MARGIN)
    h = a_shape[0] - (2 * shutter + 2 * PROCESSING_MARGIN)
    return _rect(a_shape, y, y + h, x, x + w), _rect(b_shape, y, y + h, x, x + w)


def translation_x_rects(a_shape, b_shape, tx):
    return _rect(a_shape, None, None, tx, None), _rect(b_shape, None, None, PROCESSING_MARGIN, a_shape[1] - tx + PROCESSING_MARGIN)


def translation_y_rects(a_shape, b_shape, ty):
    return _rect(a_shape, ty, None, None, None), _rect(b_shape, PROCESSING_MARGIN, a_shape[0] - ty + PROCESSING_MARGIN, None, None)


def rotation_rects(a_shape, b_shape, degree):
    h, w = b_shape
    ang = math.radians(degree)
    new_w = w * abs(math.cos(ang)) + h * abs(math.sin(ang))
    new_h = h * abs(math.cos(ang)) + w * abs(math.sin(ang))
    inner_w = w * h / new_h if w < h else h * w / new_w
    inner_h = h * w / new_w if w < h else w * h / new_h
    left, top = int((w - inner_w) / 2), int((h - inner_h) / 2)
    right, bottom = int((w + inner_w) / 2), int((h + inner_h) / 2)
    return _rect(a_shape, top, bottom, left, right), _rect(b_shape, top, bottom, left, right)


def roi_collimator(shape, shutter, b_shape=None):
    return _roi(collimator_rects(shape, b_shape or shape, shutter))


def roi_translation_x(shape, tx, b_shape=None):
    return _roi(translation_x_rects(shape, b_shape or shape, tx))


def roi_translation_y(shape, ty, b_shape=None):
    return _roi(translation_y_rects(shape, b_shape or shape, ty))


def roi_rotation(shape, degree, b_shape=None):
    return _roi(rotation_rects(shape, b_shape or shape, degree))


def register_collimator(alt, unalt, shutter):
    return _crop(alt, unalt, collimator_rects(alt.shape, unalt.shape, shutter))


def register_translation_x(alt, unalt, tx):
    return _crop(alt, unalt, translation_x_rects(alt.shape, unalt.shape, tx))


def register_translation_y(alt, unalt, ty):
    return _crop(alt, unalt, translation_y_rects(alt.shape, unalt.shape, ty))


def rotated_reference(unalt, degree):
    """The unaltered result rotated like the alteration (nearest neighbour, zero fill), what register_rotation compares against."""
    return ndimage.rotate(unalt, degree, reshape=False, order=0, mode="constant", cval=0)


def register_rotation(alt, unalt, degree):
    return _crop(alt, rotated_reference(unalt, degree), rotation_rects(alt.shape, unalt.shape, degree))


def register_symmetry(alt, unalt, element):
    """The whole altered result against the unaltered result transformed like the alteration: the margin is symmetric, so nothing is cropped."""
    return alt, apply_symmetry(unalt, element)


def roi_symmetry(shape):
    """The full frame, as the region of a device-side comparison."""
    return (0, 0, 0, 0, shape[1], shape[0])


def register_blur(alt, unalt, radius):
    """The altered result against the unaltered result blurred like the alteration, both inset by the radius: within `radius` pixels of
    the output plane's border the blurred reference is built from clamped neighbours, while the altered output there came from real
    neighbours in the processing margin."""
    r = int(radius)
    h, w = alt.shape
    return alt[r:max(h - r, r), r:max(w - r, r)], binomial_blur(unalt, r)[r:max(h - r, r), r:max(w - r, r)]


def roi_blur(shape, radius):
    """The full frame inset by the radius, as the region of a device-side comparison; None when a side falls under 7."""
    return _inset((0, 0, 0, 0, shape[1], shape[0]), int(radius))


def register_zoom(alt, unalt, ratio):
    """The whole altered result against the unaltered result magnified like the alteration: a zoom above 1 about the centre needs no
    fill and crop and zoom commute (zoom), so nothing is cropped."""
    return alt, zoom(unalt, ratio)


def roi_zoom(shape):
    """The full frame, as the region of a device-side comparison (as roi_symmetry)."""
    return (0, 0, 0, 0, shape[1], shape[0])


def register_scatter(alt, unalt, spec):
    """The altered result against the unaltered result veiled like the alteration, both inset by 2R (as register_blur, carried to low
    frequencies): within 2R pixels of the output plane's border the veiled reference is built from clamped neighbours, while the altered
    output there came from real neighbours in the processing margin."""
    r = 2 * mp.scatter_spec(spec)[0]
    h, w = alt.shape
    return alt[r:max(h - r, r), r:max(w - r, r)], scatter(unalt, spec)[r:max(h - r, r), r:max(w - r, r)]


def roi_scatter(shape, spec):
    """The full frame inset by 2R, as the region of a device-side comparison; None when a side falls under 7."""
    return _inset((0, 0, 0, 0, shape[1], shape[0]), 2 * mp.scatter_spec(spec)[0])


def register_warp(alt, unalt, field):
    """The altered result against the unaltered result warped like the alteration (the raw plane's field at the origin of the output
    plane, the margin), both inset by the field's reach: within it the warped reference is built from clamped neighbours, while the
    altered output there came from real neighbours in the processing margin (warp)."""
    r = warp_reach(field)
    h, w = alt.shape
    return alt[r:max(h - r, r), r:max(w - r, r)], warp(unalt, field, origin=(PROCESSING_MARGIN,) * 2)[r:max(h - r, r), r:max(w - r, r)]


def roi_warp(shape, field):
    """The full frame inset by the field's reach, as the region of a device-side comparison; None when a side falls under 7."""
    return _inset((0, 0, 0, 0, shape[1], shape[0]), warp_reach(field))


# ---- running the pipeline -------------------------------------------------------------------------

class Runner:
    """Processes raw images to the 8-bit output the reference's saveOutImage writes (margin cropped)."""

    def __init__(self, image_size, levels=0, device=0, use_cli=False, device_metrics=False, device_alterations=False, ensemble_batch=8):
        if use_cli and device_alterations:
            raise ValueError("device alterations write the library's resident input buffer: the CLI path has none")
        if use_cli and device_metrics:
            raise ValueError("device metrics score the library's device output: the CLI path has none")
        self.n, self.levels, self.device, self.use_cli = image_size, levels, device, use_cli
        self.device_alterations = device_alterations   # run_study generates the alterations on the device (musica_alter); implies device_metrics
        self.device_metrics = device_metrics or device_alterations   # run_study scores on the device (musica_sim_compare) instead of with numpy
        self.ensemble_batch = int(ensemble_batch)       # images per step of the ensemble context (run_study's ensemble=K)
        if self.ensemble_batch < 1:
            raise ValueError("ensemble_batch %d must be at least 1" % self.ensemble_batch)
        self.ensemble_proc = None                       # a second context of the runner's size, levels and device, created on first use
        self.proc = None
        if not use_cli:
            self.proc = mp.MusicaProcessing(device=device)
            if not self.proc.init(image_size, levels=levels):
                raise RuntimeError("musica_create failed: " + mp.last_error())

    def run(self, raw, workdir=None):
        """raw: (N, N) uint16 -> (N-20, N-20) uint8."""
        if self.use_cli:
            return self._run_cli(raw, workdir or ".")
        if not self.proc.execute(raw):
            raise RuntimeError("musica_execute failed: " + mp.last_error())
        return self.proc.out_pixels()

    def run_device(self, raw):
        """The same step, its output left on the device (for sim_capture / sim_compare)."""
        if not self.proc.execute(raw):
            raise RuntimeError("musica_execute failed: " + mp.last_error())

    def run_resident(self):
        """The step on the resident input buffer (what an alter_* call wrote), its output left on the device."""
        if not self.proc.execute_device():
            raise RuntimeError("musica_execute_device failed: " + mp.last_error())
        self.proc.sync()

    def mean_cnr(self):
        """mean(cnr image) * 256 of the last run — what test/mean_cnr/script.py prints for a cnr.bmp dump."""
        return self.proc.stats().mean_cnr

    def _run_cli(self, raw, workdir):
        """run_process of script.py:200-214: write the raw file, spawn the CLI, read the BMP back."""
        from .phantom import write_raw
        raw_path, out_path = os.path.join(workdir, "in.raw"), os.path.join(workdir, "out.bmp")
        write_raw(raw_path, raw)
        cmd = [mp.CLI_PATH, os.path.abspath(raw_path), os.path.abspath(out_path), "--size", str(self.n), "--device", str(self.device)]
        if self.levels:
            cmd += ["--levels", str(self.levels)]
        subprocess.run(cmd, check=True, capture_output=True)
        return read_bmp_gray(out_path)

    def ensemble_context(self, realisations):
        """The batch context run_study's ensembles run on, created on first use with a batch of min(ensemble_batch, realisations)."""
        if self.ensemble_proc is None:
            proc = mp.MusicaProcessing(device=self.device)
            if not proc.init(self.n, levels=self.levels, batch=max(1, min(self.ensemble_batch, int(realisations)))):
                raise RuntimeError("musica_create failed: " + mp.last_error())
            self.ensemble_proc = proc
        return self.ensemble_proc

    def close(self):
        if self.proc:
            self.proc.cleanup()
        if self.ensemble_proc:
            self.ensemble_proc.cleanup()
            self.ensemble_proc = None


def read_bmp_gray(path):
    """Reads the 24-bpp bottom-up BMP saveOutImage writes; returns the gray channel top-down."""
    b = open(path, "rb").read()
    off = int.from_bytes(b[10:14], "little")
    w, h = int.from_bytes(b[18:22], "little"), int.from_bytes(b[22:26], "little")
    row = (w * 3 + 3) & ~3
    a = np.frombuffer(b, dtype=np.uint8, count=row * h, offset=off).reshape(h, row)[:, 0:w * 3:3]
    return a[::-1].copy()


# reference slots of a device study: the unaltered result, it rotated, the vendor image, it rotated (VENDOR_SLOT: the vendor slot that
# stands beside an unaltered one)
SLOT_UNALTERED, SLOT_ROTATED, SLOT_VENDOR, SLOT_VENDOR_ROTATED = 0, 1, 2, 3
VENDOR_SLOT = {SLOT_UNALTERED: SLOT_VENDOR, SLOT_ROTATED: SLOT_VENDOR_ROTATED}
SLOT_TONE = 4   # tone=True: slots 4 .. 7 hold the slots of a row's (at most four) comparisons remapped with their tone_lut (musica_sim_remap_reference)
COMPARED = ("direct", "registered", "reference", "registered_reference")   # a row's comparisons: its own two, then the same against the vendor image
VENDOR_KEY = {"direct": "reference", "registered": "registered_reference"}   # a row's comparison -> the same against the vendor image


# The six relations of the study that measure beyond a row's comparisons, each one row of this table. key: the row key of its measurement; option / tables: run_study's
# argument with its payloads (a grid, a gain spec) and the flag that keeps the raw tables; check(payloads, n): the payloads checked for a
# raw plane of side n and, as output() maps them, for the output plane (ValueError), normalised; name(payload): the row's name;
# insert(raw, payload): the host's altered raw image; alter(proc, payload): the same on the device; output(payload): the payload in the
# coordinates of the output plane, what is measured; host(out, reference, measured) and device(proc, measured, shape): the exact
# integers of the output against the unaltered result; frame: whether summarise also takes the full frame's sq_diff_sum and pixels;
# summarise(measured, statistics, [sq_diff_sum, pixels,] tables): the row's value; source(raw): what the measurement takes from the raw
# plane itself, once per study, appended to every payload of the relation's rows (None: nothing).
Relation = collections.namedtuple("Relation", "key option tables check name insert alter output host device frame summarise source", defaults=(None,))


def _checked_grids(list_of):
    """Relation.check of a list relation: each grid is valid for the raw plane and, shifted, for the output plane."""
    def check(grids, n):
        grids = [list_of(g, n) for g in grids]
        for g in grids:
            list_of(_output_patches(g), n - 2 * PROCESSING_MARGIN)
        return grids
    return check


def _checked_gains(gains, n):
    """Relation.check of the gain relation: every spec's tables are valid for the raw plane; sliced by the margin they are for the output plane."""
    try:
        gains = [(str(name),) + tuple(tuple(int(v) for v in g) for g in mp.gain_tables(gx, gy, n)) for name, gx, gy in gains]
    except TypeError:
        raise ValueError("a gain spec is (name, gx, gy), got %r" % (gains,))
    if n <= 2 * PROCESSING_MARGIN:
        raise ValueError("a side of %d pixels leaves no output plane to take profiles of" % n)
    return gains


def _checked_luts(luts, n):
    """Relation.check of the tone-table relation: every spec is a name and a table of 65536 values in u16."""
    try:
        luts = [(str(name), mp.lut_table(lut)) for name, lut in luts]
    except TypeError:
        raise ValueError("a lut spec is (name, lut), got %r" % (luts,))
    if n <= 2 * PROCESSING_MARGIN:
        raise ValueError("a side of %d pixels leaves no output plane to take levels of" % n)
    return luts


def _frame(shape):
    return (0, 0, 0, 0, shape[1], shape[0])


RELATIONS = (
    Relation("details", "details", "detail_tables", _checked_grids(mp.detail_list), lambda g: "cd_%d" % g[0][3], insert_details,
             lambda p, g: p.alter_details(g), _output_patches, detail_statistics,
             lambda p, m, shape: p.sim_details(m, SLOT_UNALTERED), True, detail_row),
    Relation("edges", "edges", "edge_tables", _checked_grids(mp.edge_list), lambda g: "edge_%d" % g[0][6], insert_edges,
             lambda p, g: p.alter_edges(g), _output_patches, edge_statistics,
             lambda p, m, shape: p.sim_edges(m, SLOT_UNALTERED), True, edge_row),
    Relation("gratings", "gratings", "grating_tables", _checked_grids(mp.grating_list), lambda g: "grating_%d" % grating_contrast(g),
             insert_gratings, lambda p, g: p.alter_gratings(g), _output_patches, grating_statistics,
             lambda p, m, shape: p.sim_gratings(m, SLOT_UNALTERED), True, grating_row),
    # the profiles are taken over the full output frame; measured: (gx, gy) sliced into it
    Relation("profiles", "gains", "gain_tables", _checked_gains, lambda g: g[0], lambda raw, g: apply_gain(raw, g[1], g[2]), lambda p, g: p.alter_gain(g[1], g[2]),
             output_gain, lambda out, ref, m: profile_statistics(out, ref, [_frame(out.shape)])[0],
             lambda p, m, shape: p.sim_profiles([(0, SLOT_UNALTERED) + _frame(shape)])[0], False, lambda m, stats, tables: profile_row(stats, m[0], m[1], tables)),
    # the levels are taken over the full output frame; a payload: (name, lut, (shift, the class plane)), measured: the pair the study's raw plane gave
    Relation("levels", "luts", "lut_tables", _checked_luts, lambda s: s[0], lambda raw, s: apply_lut(raw, s[1]), lambda p, s: p.alter_lut(s[1]),
             lambda s: s[2], lambda out, ref, m: level_statistics(out, ref, m[1], [_frame(out.shape)], mp.level_count(m[0]))[0],
             lambda p, m, shape: p.sim_levels([(0, SLOT_UNALTERED) + _frame(shape)], m[0])[0]["table"], True,
             lambda m, table, sq_diff_sum, pixels, tables: level_row(table, sq_diff_sum, pixels, tables),
             lambda raw: (level_shift(raw), level_classes(raw, level_shift(raw)))),
    # the fourth list relation, behind the others so that its rows come last; a row is named after its grid's first contrast
    Relation("points", "points", "point_tables", _checked_grids(mp.point_list), lambda g: "point_%d" % g[0][4], insert_points,
             lambda p, g: p.alter_points(g), _output_patches, point_statistics,
             lambda p, m, shape: p.sim_points(m, SLOT_UNALTERED), True, point_row),
)


def _sides(out, plane, region):
    """The two crops of a comparison: the output by the region's a side, the reference plane by its b side."""
    ax, ay, bx, by, w, h = region
    return out[ay:ay + h, ax:ax + w], plane[by:by + h, bx:bx + w]


def _checked_flag(name):
    def check(value):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError("%s is a flag, got %r" % (name, value))
        return bool(value)
    return check


def _checked_scales(scales):
    scales = int(scales)
    if scales and not 1 <= scales <= mp.SIM_MAX_SCALES:
        raise ValueError("scales %d is not in 1 .. %d" % (scales, mp.SIM_MAX_SCALES))
    return scales


def _checked_lattice(lattice):
    if isinstance(lattice, (bool, np.bool_, str)) or not isinstance(lattice, (int, float, np.integer, np.floating)) or lattice != int(lattice):
        raise ValueError("lattice is a period, one of %r, or 0, got %r" % (LATTICE_PERIODS, lattice))
    if int(lattice):
        mp.lattice_period(int(lattice), PROCESSING_MARGIN % int(lattice))
    return int(lattice)


def _host_scales(opt, out, plane, region):
    r = multiscale_similarities(*_sides(out, plane, region), min(opt.scales, max_scales(region[4], region[5])))
    return {k: r[k] for k in SCALES_KEYS}


def _device_tone(proc, queries, opt):
    """One musica_sim_joint call, every comparison's slot remapped with its tone_lut into a slot of its own from SLOT_TONE on (a row
    has at most four), then one musica_sim_compare call over the same regions for tone_ssim."""
    res = proc.sim_joint(queries)
    for i, (q, r) in enumerate(zip(queries, res)):
        proc.sim_remap_reference(SLOT_TONE + i, q[1], r["tone_lut"])
    scored = proc.sim_compare([(0, SLOT_TONE + i) + q[2:] for i, q in enumerate(queries)])
    for r, c in zip(res, scored):
        r["tone_ssim"] = c["ssim"]
    return [{k: r[k] for k in mp.JOINT_METRICS} for r in res]


def _device_scales(proc, queries, opt):
    """One musica_sim_multiscale call per distinct scale count, ascending; the results in the comparisons' order."""
    counts = [min(opt.scales, max_scales(q[6], q[7])) for q in queries]
    out = [None] * len(queries)
    for n in sorted(set(counts)):
        idx = [i for i, c in enumerate(counts) if c == n]
        for i, r in zip(idx, proc.sim_multiscale([queries[i] for i in idx], n)):
            out[i] = {k: r[k] for k in SCALES_KEYS}
    return out


# The metrics that score every comparison of a row, each one entry of a table, in SCORING order: the order of a row's calls.
# option: run_study's argument; suffix: comparison <c> of a row (COMPARED) gets the sibling key <c>_<suffix>; on(value): whether the
# normalised option asks for the metric; check(value): the option checked (ValueError) and normalised; host(opt, out, plane, region):
# one comparison's value, the restatement on the output and the reference plane; device(proc, queries, opt): the values of a row's
# comparisons, given as musica_sim_compare's queries, from one musica_sim_* call (at most four: BLOBS_MAX_QUERIES; tone and scales make
# a few calls and keep a function each); csv: its file (report.METRIC_CSVS). Host and device summarise with one *_row function.
ComparisonMetric = collections.namedtuple("ComparisonMetric", "option suffix on check host device csv")
COMPARISON_METRICS = (
    ComparisonMetric("tone", "tone", bool, lambda v: v, lambda opt, out, plane, region: tone_similarities(*_sides(out, plane, region)),
                     _device_tone, METRIC_CSVS["tone"]),
    ComparisonMetric("scales", "scales", bool, _checked_scales, _host_scales, _device_scales, METRIC_CSVS["scales"]),
    ComparisonMetric("gradients", "gradient", bool, _checked_flag("gradients"),
                     lambda opt, out, plane, region: gradient_row(*gradient_statistics(out, plane, [region])[0]),
                     lambda proc, queries, opt: [gradient_row(r["table"], r["gsim"]) for r in proc.sim_gradients(queries)], METRIC_CSVS["gradient"]),
    ComparisonMetric("order", "order", bool, _checked_flag("order"),
                     lambda opt, out, plane, region: order_row(order_statistics(out, plane, [region])[0]),
                     lambda proc, queries, opt: [order_row(np.concatenate([r["rings"].ravel(), r["histogram"]])) for r in proc.sim_order(queries)],
                     METRIC_CSVS["order"]),
    ComparisonMetric("lattice", "lattice", bool, _checked_lattice,
                     lambda opt, out, plane, region: lattice_row(lattice_statistics(out, plane, [region], opt.lattice, PROCESSING_MARGIN % opt.lattice)[0]),
                     lambda proc, queries, opt: [lattice_row(r["table"]) for r in proc.sim_lattice(queries, opt.lattice, PROCESSING_MARGIN % opt.lattice)],
                     METRIC_CSVS["lattice"]),
    ComparisonMetric("blobs", "blobs", lambda v: v is not None, lambda v: None if v is None else mp.blob_threshold(v),
                     lambda opt, out, plane, region: blob_row(blob_statistics(out, plane, [region], opt.blobs, opt.blob_connectivity)[0]),
                     lambda proc, queries, opt: [blob_row(r) for r in proc.sim_blobs(queries, opt.blobs, opt.blob_connectivity)], METRIC_CSVS["blobs"]),
    ComparisonMetric("spectrum", "spectrum", lambda v: v is not None, lambda v: None if v is None else mp.spectrum_tile(v),
                     lambda opt, out, plane, region: spectrum_row(spectrum_statistics(out, plane, [region], opt.spectrum)[0], opt.spectrum),
                     lambda proc, queries, opt: [spectrum_row(r, opt.spectrum) for r in proc.sim_spectrum(queries, opt.spectrum)], METRIC_CSVS["spectrum"]),
)
# COMPARISON_METRICS is the seven entries above and ends with the spectrum: tests/test_spectrum_restatement.py holds it to that. The
# study walks STUDY_METRICS, the same table with the metrics added since appended, in scoring order.
STUDY_METRICS = COMPARISON_METRICS + (
    ComparisonMetric("texture", "texture", lambda v: v is not None, lambda v: None if v is None else mp.cooccurrence_levels(v),
                     lambda opt, out, plane, region: texture_row(cooccurrence_statistics(out, plane, [region], opt.texture, opt.texture_distances)[0], opt.texture, opt.texture_distances),
                     lambda proc, queries, opt: [texture_row(r, opt.texture, opt.texture_distances) for r in proc.sim_cooccurrence(queries, opt.texture, opt.texture_distances)],
                     METRIC_CSVS["texture"]),
)
# STUDY_METRICS is the eight entries above and ends with the texture: tests/test_cooccurrence_restatement.py holds it to that. The
# granulometry and the contours are appended in ROW_METRICS, which tests/test_contours_restatement.py holds to end with the contours.
ROW_METRICS = STUDY_METRICS + (
    ComparisonMetric("granulometry", "granulometry", lambda v: v is not None, lambda v: None if v is None else mp.granulometry_radii(v),
                     lambda opt, out, plane, region: granulometry_row(granulometry_statistics(out, plane, [region], opt.granulometry)[0], opt.granulometry),
                     lambda proc, queries, opt: [granulometry_row(r, opt.granulometry) for r in proc.sim_granulometry(queries, opt.granulometry)],
                     METRIC_CSVS["granulometry"]),
    ComparisonMetric("contours", "contours", lambda v: v is not None, lambda v: None if v is None else mp.contour_threshold(v),
                     lambda opt, out, plane, region: contour_row(contour_statistics(out, plane, [region], opt.contours, opt.contour_radius, planes=opt.contour_maps)[0],
                                                                 opt.contours, opt.contour_radius),
                     lambda proc, queries, opt: [contour_row(r, opt.contours, opt.contour_radius)
                                                 for r in proc.sim_contours(queries, opt.contours, opt.contour_radius, planes=opt.contour_maps)],
                     METRIC_CSVS["contours"]),
)
# ROW_METRICS is the ten entries above and ends with the contours: tests/test_contours_restatement.py holds it to that. The study, its
# checks, its key groups, the command line and the report walk SCORED_METRICS (and report.SCORED_CSVS), the same table with the metrics
# added since appended, in scoring order. The tests of a new metric hold this table by MEMBERSHIP AND PREFIX (ROW_METRICS is its prefix;
# exactly one entry has the metric's option), never by its last element: the next metric is appended HERE and nothing is renamed again.
SCORED_METRICS = ROW_METRICS + (
    ComparisonMetric("minkowski", "minkowski", bool, _checked_flag("minkowski"),
                     lambda opt, out, plane, region: minkowski_row(minkowski_statistics(out, plane, [region])[0], opt.minkowski_curves),
                     lambda proc, queries, opt: [minkowski_row(r, opt.minkowski_curves) for r in proc.sim_minkowski(queries)],
                     SCORED_CSVS["minkowski"]),
)
TONE_KEYS, SCALE_ROW_KEYS, GRADIENT_ROW_KEYS, ORDER_ROW_KEYS, LATTICE_ROW_KEYS, BLOB_ROW_KEYS = \
    ({c: "%s_%s" % (c, m.suffix) for c in COMPARED} for m in COMPARISON_METRICS[:6])   # comparison -> its sibling key, of the metrics that tests ask by name
# The order of the refusals and of a row's keys is history, not the scoring order. These metrics are checked before the moved rows'
# options, every other one behind them; the key groups stand in this order, a metric that is not named behind them all.
CHECKED_EARLY = ("scales", "gradients", "order")
KEY_GROUPS = ("tone", "shift", "scales", "gradient", "order", "reach", "ensemble", "relations", "observer", "warp", "lattice", "blobs")


def _checked_ints(what, lo, hi):
    """Moved.check of a list of integers lo .. hi: all converted, then each checked."""
    def check(values, n):
        values = [int(v) for v in values]
        for v in values:
            if not lo <= v <= hi:
                raise ValueError("%s %d is not in %d .. %d" % (what, v, lo, hi))
        return values
    return check


def _checked_warps(warps, n):
    try:
        warps = [(str(name), mp.warp_field(field, n)) for name, field in warps]
    except TypeError:
        raise ValueError("a warp spec is (name, field), got %r" % (warps,))
    for _, field in warps:   # the same nodes at the origin of the output plane
        if n <= 2 * PROCESSING_MARGIN:
            raise ValueError("a side of %d pixels leaves no output plane to warp" % n)
        mp.warp_field(field, n - 2 * PROCESSING_MARGIN, PROCESSING_MARGIN)
    return warps


def _checked_codecs(codecs, n):
    try:
        codecs = [int(s) for s in codecs]
    except (TypeError, ValueError):
        raise ValueError("codecs is a list of DC steps, got %r" % (codecs,))
    for s in codecs:
        codec_table(s)
    if codecs and n <= 2 * PROCESSING_MARGIN:
        raise ValueError("a side of %d pixels leaves no output plane to compress" % n)
    return codecs


# The six alterations that move a reference plane the way they move the input, each one entry of this table, in the rows' order (and
# the refusals'). option: run_study's argument, a list of values; name(v): the row's name; check(values, n): the list checked for a raw
# plane of side n (ValueError) and normalised; host(raw, v): the altered raw image; alter(proc, v): the same on the device;
# region(shape, v): the region of the registered comparison; move(v): Alteration.move, (the context's sim_*_reference method, the
# host's function of the output plane, their parameter); field(v): Alteration.warp; cli(v, n): --<option>'s value as run_study's.
Moved = collections.namedtuple("Moved", "option name check host alter region move field cli", defaults=(None, None))
MOVED = (
    Moved("symmetries", lambda e: "d4_%d" % e, _checked_ints("symmetry element", 0, 7), apply_symmetry, lambda p, e: p.alter_symmetry(e),
          lambda shape, e: roi_symmetry(shape), lambda e: ("sim_transform_reference", apply_symmetry, e)),
    Moved("blurs", lambda r: "blur_%d" % r, _checked_ints("blur radius", 1, mp.BLUR_MAX_RADIUS), binomial_blur, lambda p, r: p.alter_blur(r), roi_blur,
          lambda r: ("sim_blur_reference", binomial_blur, r)),
    Moved("zooms", lambda z: "zoom_%d_%d" % z, lambda zooms, n: [mp.zoom_ratio(z) for z in zooms], zoom, lambda p, z: p.alter_zoom(z),
          lambda shape, z: roi_zoom(shape), lambda z: ("sim_zoom_reference", zoom, z)),
    Moved("scatters", lambda s: "scatter_%d_%d_%d" % s, lambda scatters, n: [mp.scatter_spec(s) for s in scatters], scatter, lambda p, s: p.alter_scatter(s), roi_scatter,
          lambda s: ("sim_scatter_reference", scatter, s), cli=lambda v, n: SCATTERS(n) if v is True else v),
    # a value: the spec (name, field); the output plane's origin on the control grid is the margin
    Moved("warps", lambda w: w[0], _checked_warps, lambda raw, w: warp(raw, w[1]), lambda p, w: p.alter_warp(w[1]), lambda shape, w: roi_warp(shape, w[1]),
          lambda w: ("sim_warp_reference", lambda plane, f: warp(plane, f, origin=(PROCESSING_MARGIN,) * 2), w[1]), lambda w: w[1],
          lambda v, n: [w for w in WARPS(n) if v is True or w[0] in v]),
    # a value: the DC step; the output plane's blocks lie where the raw plane's lay, its origin is the margin mod 8, its table the 8-bit one
    Moved("codecs", lambda s: "codec_%d" % s, _checked_codecs, lambda raw, s: block_codec(raw, codec_table(s)), lambda p, s: p.alter_codec(codec_table(s)),
          lambda shape, s: _frame(shape),
          lambda s: ("sim_codec_reference", lambda plane, t: block_codec(plane, t, (PROCESSING_MARGIN % 8,) * 2), codec_table8(codec_table(s)))),
)


def study_options(n, runner, shutters, translations, rotations, sigmas, factors, vendor, symmetries, tone, displacement, displacement_tiles,
                  scales, ensemble, ensemble_tiles, covariance, covariance_tiles, blurs, zooms=None, scatters=None, details=None,
                  detail_tables=False, edges=None, edge_tables=False, gratings=None, grating_tables=False, gains=None, gain_tables=False, luts=None, lut_tables=False, warps=None,
                  gradients=False, points=None, point_tables=False, reach=None, reach_tables=False, reach_maps=False, observer=False, codecs=None,
                  lattice=0, blobs=None, blob_connectivity=8, spectrum=None, texture=None, texture_distances=mp.COOCCURRENCE_DISTANCES, granulometry=None, contours=None, contour_radius=mp.CONTOURS_RADIUS, contour_maps=False, minkowski=False, minkowski_curves=False, order=False):
    """run_study's arguments for a raw image of side n, checked in this order before any work (ValueError; the runner is only asked for
    its device_alterations) and normalised: a namespace of them, the grids' defaults filled in, plus `keys` (the keys of a row, in
    order) and `device_alterations`."""
    o = {k: v for k, v in locals().items() if k not in ("n", "runner")}   # every option by its name: checked and normalised in place, the namespace in the end
    if vendor is not None:
        o["vendor"] = vendor = np.asarray(vendor)
        want = (n - 2 * PROCESSING_MARGIN,) * 2
        if vendor.shape != want or vendor.dtype not in (np.uint8, np.uint16):
            raise ValueError("vendor image must be a %d x %d uint8 or uint16 array, got %r %s" % (want + (vendor.shape, vendor.dtype)))
    o["displacement"] = displacement = int(displacement)
    if displacement and not 1 <= displacement <= mp.SIM_MAX_RADIUS:
        raise ValueError("displacement radius %d is not in 1 .. %d" % (displacement, mp.SIM_MAX_RADIUS))
    for m in SCORED_METRICS:
        if m.option in CHECKED_EARLY:
            o[m.option] = m.check(o[m.option])
    o["observer"] = _checked_flag("observer")(observer)
    if observer and details is None:
        raise ValueError("the observer looks at the details of the cd_ rows: give details")
    o["reach"] = None if reach is None or reach is False else [int(r) for r in mp.reach_radii(REACH_RADII(n) if reach is True else reach)]
    o["ensemble"] = ensemble = int(ensemble)
    device_alterations = getattr(runner, "device_alterations", False)
    if ensemble and not 1 <= ensemble <= mp.SIM_ENSEMBLE_MAX:
        raise ValueError("ensemble %d is not in 1 .. %d" % (ensemble, mp.SIM_ENSEMBLE_MAX))
    if ensemble and not device_alterations:
        raise ValueError("an ensemble repeats the device's noise alterations: it needs a runner with device_alterations")
    o["covariance"] = covariance = int(covariance)
    if covariance and not 1 <= covariance <= mp.SIM_MAX_RADIUS:
        raise ValueError("covariance radius %d is not in 1 .. %d" % (covariance, mp.SIM_MAX_RADIUS))
    if covariance and not ensemble:
        raise ValueError("covariance is taken over the realisations of an ensemble: give ensemble > 0")
    for m in MOVED:
        o[m.option] = m.check(o[m.option] or (), n)
    for m in SCORED_METRICS:
        if m.option not in CHECKED_EARLY:
            o[m.option] = m.check(o[m.option])
    if blob_connectivity not in (4, 8) or isinstance(blob_connectivity, (bool, np.bool_)):
        raise ValueError("blob_connectivity is 4 or 8, got %r" % (blob_connectivity,))
    o["blob_connectivity"] = int(blob_connectivity)
    o["texture_distances"] = mp.cooccurrence_distances(texture_distances)
    o["contour_radius"] = mp.contour_radius(contour_radius)
    o["contour_maps"] = _checked_flag("contour_maps")(contour_maps)
    o["minkowski_curves"] = _checked_flag("minkowski_curves")(minkowski_curves)
    for rel in RELATIONS:
        if o[rel.option] is not None:
            o[rel.option] = rel.check(o[rel.option], n)
    for g in (o["details"] if observer else ()):   # the views and banks of every grid, as the measurement will take them
        mp.view_list(*observer_views(output_details(g)), n - 2 * PROCESSING_MARGIN)
    compared = COMPARED[:2 if vendor is None else 4]
    groups = {m.suffix: tuple("%s_%s" % (c, m.suffix) for c in compared) if m.on(o[m.option]) else () for m in SCORED_METRICS}
    groups.update(shift=("direct_shift", "registered_shift") if displacement else (), reach=("direct_reach",) if o["reach"] is not None else (),
                  ensemble=("ensemble",) if ensemble else (), relations=tuple(rel.key for rel in RELATIONS if o[rel.option] is not None),
                  observer=("observer",) if observer else (), warp=("warp",) if o["warps"] else ())
    keys = ("alteration", "direct", "registered", "mean_cnr") + compared[2:] + \
           tuple(k for g in KEY_GROUPS + tuple(m.suffix for m in SCORED_METRICS if m.suffix not in KEY_GROUPS) for k in groups[g])
    for grid, default in (("shutters", scaled(SHUTTERS, n)), ("translations", scaled(TRANSLATIONS, n)), ("rotations", ROTATIONS),
                          ("sigmas", GAUSS_SIGMAS), ("factors", POISSON_FACTORS)):
        if o[grid] is None:
            o[grid] = default
    for rel in RELATIONS:
        o[rel.option], o[rel.tables] = o[rel.option] or [], bool(o[rel.tables])
    o["reach_tables"], o["reach_maps"] = bool(reach_tables), bool(reach_maps)
    return types.SimpleNamespace(keys=keys, device_alterations=device_alterations, **o)


# One alteration of the study: its row's name; host() the altered raw image; dev() the call that writes it into the resident input buffer;
# region() the region of the registered comparison (None, or no region at all as for the noise rows: no registration); move = (the
# context's method, the host's function, their parameter), which both move a reference plane as the alteration moves the input: the
# registered comparison is then against the moved plane; noise = (the row's ordinal, alter(context, stream, image_index)) for the rows
# that draw, what their ensembles repeat; measure = (relation, payload) for the rows of a relation (RELATIONS): what the row
# measures beyond its comparisons, the raw plane's grid, gain spec or lut spec (with what Relation.source took from the raw plane); warp:
# the field of a warp row, what its "warp" key reports and tracks.
Alteration = collections.namedtuple("Alteration", "name host dev region move noise measure warp", defaults=(None, None, None, None, None))


def study_alterations(raw, rng, p, seed, shape, opt):
    """Every Alteration of the study once, in the rows' order. run_study makes a row's calls before the next one is built: the rows'
    order is the order of the `rng` draws. The device's noise draws (context p, the study's seed) take the row's ordinal in the study
    as their stream; the d4, blur, zoom, scatter, warp, codec, cd, edge, grating, gain and lut rows draw nothing and take no ordinal."""
    ordinal = itertools.count(1)
    for s in opt.shutters:
        k = next(ordinal)
        yield Alteration("c_sh_%d" % s, lambda: apply_collimator(raw, s, s, rng), lambda k=k: p.alter_collimator(s, s, seed, k),
                         lambda: roi_collimator(shape, s), noise=(k, lambda q, stream, i: q.alter_collimator(s, s, seed, stream, i)))
    for name, tx, ty, roi in (("t_x_%d", 1, 0, roi_translation_x), ("t_y_%d", 0, 1, roi_translation_y)):
        for t in opt.translations:
            next(ordinal)   # every row before the d4 rows takes one, drawing or not
            yield Alteration(name % t, lambda: clamp_translation(raw, tx * t, ty * t), lambda: p.alter_translate(tx * t, ty * t),
                             lambda: roi(shape, t))
    for d in opt.rotations:
        next(ordinal)
        yield Alteration("r_%d" % d, lambda: clamp_rotate(raw, d), lambda: p.alter_rotate(d), lambda: roi_rotation(shape, d),
                         ("sim_rotate_reference", rotated_reference, d))
    for sg in opt.sigmas:
        k = next(ordinal)
        yield Alteration("gn_%s" % sg, lambda: add_gaussian_noise(raw, 0.0, sg, rng), lambda k=k: p.alter_gaussian(0.0, sg, seed, k),
                         noise=(k, lambda q, stream, i: q.alter_gaussian(0.0, sg, seed, stream, i)))
    for f in opt.factors:
        k = next(ordinal)
        yield Alteration("pn_%s" % f, lambda: apply_quantum_noise(raw, f, rng), lambda k=k: p.alter_poisson(f, seed, k),
                         noise=(k, lambda q, stream, i: q.alter_poisson(f, seed, stream, i)))
    for m in MOVED:
        for v in getattr(opt, m.option):
            yield Alteration(m.name(v), lambda: m.host(raw, v), lambda: m.alter(p, v), lambda: m.region(shape, v), m.move(v),
                             warp=m.field(v) if m.field else None)
    for rel in RELATIONS:
        payloads = getattr(opt, rel.option)
        carried = (rel.source(raw),) if rel.source and payloads else ()
        for g in (tuple(g) + carried if carried else g for g in payloads):
            yield Alteration(rel.name(g), lambda: rel.insert(raw, g), lambda: rel.alter(p, g), measure=(rel, g))


class Scorer:
    """How run_study scores a row, on the host or on the device. produce(alteration) makes the altered output the one that is scored
    (until then it is the unaltered result); move(method, function, parameter) moves the unaltered result, and the vendor image, into
    SLOT_ROTATED and SLOT_VENDOR_ROTATED; measure(relation, measured) gives the value of a patch relation's row key and
    observer(details) a cd_ row's "observer". similarities, score and shifts take the row's comparisons, (reference key, region) pairs
    with a SLOT_* number as the key, and return one result each: similarities the five SIM_METRICS, score(metric, comparisons) the
    sibling values of one entry of SCORED_METRICS, by the entry's host or device form, and shifts the displacement (the regions
    already inset; keep: the dicts carry their tile tables whatever displacement_tiles says, for a warp row's tracking). reach takes
    the row's direct comparison, behind similarities, and looks at the change of the input from `source`, the study's raw plane."""

    def __init__(self, runner, opt, unalt):
        self.runner, self.proc, self.opt, self.unalt = runner, runner.proc, opt, unalt

    def shift_summary(self, table, region, tiles, tiles_off, tile_tables, keep=False):
        out = displacement_summary(table, region[4] * region[5], tiles, tiles_off)
        if self.opt.displacement_tiles or keep:
            out["tile_tables"], out["size"] = tile_tables, (region[4], region[5])
        return out

    def reach_value(self, table, seeds, sq_diff_sum, pixels, class_plane=None):
        """A row's direct_reach from a full-frame reach table: None where the alteration changed no input pixel, or every one. With
        reach_maps the output's class plane rides along."""
        if not 0 < seeds < self.source.size:
            return None
        out = reach_row(table, self.opt.reach, seeds, sq_diff_sum, pixels, self.opt.reach_tables)
        if self.opt.reach_maps and class_plane is not None:
            out["class_plane"] = np.asarray(class_plane)
        return out


class DeviceScorer(Scorer):
    """The output is image 0 of the runner's context, a reference key the slot itself: every method is one or a few sim_* calls."""

    def __init__(self, runner, opt, unalt):
        super().__init__(runner, opt, unalt)
        self.proc.sim_capture(SLOT_UNALTERED)
        if opt.vendor is not None:
            self.proc.sim_set_vendor_reference(SLOT_VENDOR, opt.vendor)

    def produce(self, alteration):
        if self.opt.device_alterations:
            alteration.dev()
            self.runner.run_resident()
        else:
            self.runner.run_device(alteration.host())

    def move(self, method, function, parameter):
        if self.opt.device_alterations:
            getattr(self.proc, method)(SLOT_ROTATED, SLOT_UNALTERED, parameter)
        else:
            self.proc.sim_set_reference(SLOT_ROTATED, function(self.unalt, parameter))
        if self.opt.vendor is not None:
            getattr(self.proc, method)(SLOT_VENDOR_ROTATED, SLOT_VENDOR, parameter)

    def similarities(self, comparisons):
        self.compared = self.proc.sim_compare([(0, slot) + region for slot, region in comparisons])   # measure() reads the direct one's integers
        return [{k: r[k] for k in mp.SIM_METRICS} for r in self.compared]

    def measure(self, relation, measured):
        """One call of the relation's musica_sim_* against the unaltered result; the full frame's integers are the row's direct comparison's."""
        direct = self.compared[0]
        frame = (direct["sq_diff_sum"], direct["pixels"]) if relation.frame else ()
        return relation.summarise(measured, relation.device(self.proc, measured, self.unalt.shape), *frame, getattr(self.opt, relation.tables))

    def observer(self, details):
        """One musica_sim_observer call behind the row's musica_sim_details: the details' views against the unaltered result."""
        views, banks = observer_views(details)
        return observer_row(details, self.proc.sim_observer(views, banks, SLOT_UNALTERED))

    def score(self, metric, comparisons):
        """The metric's musica_sim_* call, or calls, over the row's comparisons as musica_sim_compare's queries."""
        return metric.device(self.proc, [(0, slot) + region for slot, region in comparisons], self.opt)

    def reach(self, comparisons):
        """One musica_sim_reach call over the row's direct comparison (the first that similarities() scored)."""
        res = self.proc.sim_reach([(0, slot) + region for slot, region in comparisons], self.opt.reach)
        plane = self.proc.sim_reach_classes(self.opt.reach) if self.opt.reach_maps else None
        return [self.reach_value(r["table"], r["seeds"], self.compared[i]["sq_diff_sum"], self.compared[i]["pixels"], plane) for i, r in enumerate(res)]

    def shifts(self, comparisons, keep=False):
        """One musica_sim_displace call, none without a comparison."""
        res = self.proc.sim_displace([(0, slot) + region for slot, region in comparisons], self.opt.displacement, tables=True,
                                     tiles=self.opt.displacement_tiles or keep) if comparisons else []
        return [self.shift_summary(r["table"], region, r["tiles_x"] * r["tiles_y"], r["tiles_off"], r.get("tile_tables"), keep)
                for (_, region), r in zip(comparisons, res)]


class HostScorer(Scorer):
    """The output is an array and a reference key looks up a full plane (the unaltered result, the vendor image as vendor_to_u8 converts
    it, and what move() made of them): every comparison is the restatement on the output cropped by the region's a side and the plane
    cropped by its b side."""

    def __init__(self, runner, opt, unalt):
        super().__init__(runner, opt, unalt)
        self.out = unalt
        self.planes = {SLOT_UNALTERED: unalt}
        if opt.vendor is not None:
            self.planes[SLOT_VENDOR] = vendor_to_u8(opt.vendor)

    def produce(self, alteration):
        self.altered = alteration.host()
        self.out = self.runner.run(self.altered)

    def move(self, method, function, parameter):
        for slot, moved in ((SLOT_UNALTERED, SLOT_ROTATED), (SLOT_VENDOR, SLOT_VENDOR_ROTATED)):
            if slot in self.planes:
                self.planes[moved] = function(self.planes[slot], parameter)

    def similarities(self, comparisons):
        return [similarities(*_sides(self.out, self.planes[slot], region)) for slot, region in comparisons]

    def measure(self, relation, measured):
        frame = ()
        if relation.frame:
            a, b = self.out.astype(np.int64), self.planes[SLOT_UNALTERED].astype(np.int64)
            frame = (int(((a - b) ** 2).sum()), a.size)
        return relation.summarise(measured, relation.host(self.out, self.planes[SLOT_UNALTERED], measured), *frame, getattr(self.opt, relation.tables))

    def observer(self, details):
        views, banks = observer_views(details)
        return observer_row(details, channel_responses(self.out, self.planes[SLOT_UNALTERED], views, banks))

    def score(self, metric, comparisons):
        return [metric.host(self.opt, self.out, self.planes[slot], region) for slot, region in comparisons]

    def reach(self, comparisons):
        """The restatement on the altered input that produce() kept."""
        classes = reach_classes(self.source, self.altered, self.opt.reach)
        seeds, out = int(np.count_nonzero(self.source != self.altered)), []
        for slot, region in comparisons:
            table, = reach_statistics(self.out, self.planes[slot], classes, [region], len(self.opt.reach) + 1)
            a, b = (p.astype(np.int64) for p in _sides(self.out, self.planes[slot], region))
            out.append(self.reach_value(table, seeds, int(((a - b) ** 2).sum()), a.size, classes[PROCESSING_MARGIN:-PROCESSING_MARGIN, PROCESSING_MARGIN:-PROCESSING_MARGIN]))
        return out

    def shifts(self, comparisons, keep=False):
        tables = [(region, displacement_tile_tables(self.out, self.planes[slot], region, self.opt.displacement)) for slot, region in comparisons]
        return [self.shift_summary(tt.astype(np.int64).sum(axis=(0, 1)), region, tt.shape[0] * tt.shape[1], displacement_tiles_off(tt), tt, keep)
                for region, tt in tables]


def ensemble_of(eproc, noise, registered, full, opt):
    """The "ensemble" value of a completed row, on the ensemble context: None unless it is a noise row (noise: its Alteration's).
    registered: the region of its registered comparison (None: the row has none)."""
    if noise is None:
        return None
    ordinal, alter = noise
    ensemble, covariance = opt.ensemble, opt.covariance
    regions = [full] + ([registered] if registered is not None else [])
    per = {k: [] for k in mp.SIM_METRICS}
    eproc.sim_ensemble_reset()
    if covariance:
        tracked = [_inset(full, covariance), _inset(registered, covariance) if registered is not None else None]
        if tracked[0] is None:
            raise ValueError("covariance radius %d leaves no 7 x 7 region of the %d x %d output" % (covariance, full[4], full[5]))
        eproc.sim_ensemble_track([(0, SLOT_UNALTERED) + r for r in tracked if r is not None], covariance)
    for j0 in range(0, ensemble, eproc.batch):
        count = min(eproc.batch, ensemble - j0)
        for i in range(count):
            alter(eproc, ensemble_stream(ordinal, j0 + i), i)
        if not eproc.execute_device():
            raise RuntimeError("musica_execute_device failed: " + mp.last_error())
        eproc.sim_ensemble_add(0, count)
        for r in eproc.sim_compare([(i, SLOT_UNALTERED) + full for i in range(count)]):
            for k in mp.SIM_METRICS:
                per[k].append(r[k])
    res = eproc.sim_ensemble_result([(0, SLOT_UNALTERED) + r for r in regions], tiles=opt.ensemble_tiles)
    dicts = [ensemble_summary(*[r[k] for k in ("sq_bias_sum", "var_sum", "sq_err_sum", "bias_sum", "abs_bias_max", "var_max", "realisations")],
                              g[4], g[5]) for r, g in zip(res, regions)]
    if opt.ensemble_tiles:
        dicts[0]["tile_tables"], dicts[0]["size"] = res[0]["tile_tables"], (full[4], full[5])
    out = {"direct": dicts[0], "registered": dicts[1] if registered is not None else None, "realisations": ensemble,
           "per_realisation": {"mean": {k: float(np.mean(v)) for k, v in per.items()},
                               "std": {k: float(np.std(v, ddof=1)) if ensemble > 1 else 0.0 for k, v in per.items()}}}
    if covariance:
        cov = iter(eproc.sim_ensemble_covariance(tables=True, tiles=opt.covariance_tiles))
        groups = []
        for r in tracked:
            if r is None:
                groups.append(None)
                continue
            c = next(cov)
            d = covariance_row(c["table"], c["realisations"], r[4], r[5])
            if opt.covariance_tiles:
                d["table"], d["tile_tables"] = c["table"], c["tile_tables"]
            groups.append(d)
        out["covariance"] = {"direct": groups[0], "registered": groups[1]}
    return out


def run_study(raw, runner, rng=None, shutters=None, translations=None, rotations=None, sigmas=None, factors=None, vendor=None, symmetries=None,
              tone=False, displacement=0, displacement_tiles=False, scales=0, ensemble=0, ensemble_tiles=False, covariance=0, covariance_tiles=False,
              blurs=None, zooms=None, scatters=None, details=None, detail_tables=False, edges=None, edge_tables=False, gratings=None, grating_tables=False,
              gains=None, gain_tables=False, luts=None, lut_tables=False, warps=None, gradients=False, points=None, point_tables=False, reach=None,
              reach_tables=False, reach_maps=False, observer=False, codecs=None, lattice=0, blobs=None, blob_connectivity=8, spectrum=None, texture=None, texture_distances=mp.COOCCURRENCE_DISTANCES, granulometry=None, contours=None, contour_radius=mp.CONTOURS_RADIUS, contour_maps=False, minkowski=False, minkowski_curves=False, order=False):
    """The reference's per-image loop (script.py:383-657): returns a list of rows
    {alteration, direct: {...}, registered: {...} or None, mean_cnr}. With runner.device_metrics the similarities are computed
    on the device against the unaltered result kept in reference slot 0 (rotations: the rotated unaltered result in slot 1).

    With runner.device_alterations the raw image is uploaded once and every alteration is generated on the device (musica_alter),
    the rotated unaltered result comes from musica_sim_rotate_reference, and the seed of the noise alterations is drawn from `rng`, their
    ordinal in the study being the stream. The geometric alterations are bit-identical to the host's, so their rows equal a device-metrics
    study's; the noise rows (c_sh_*, gn_*, pn_*) come from a different, reproducible, stream than the host study's numpy draws.

    vendor: the vendor-processed image of `raw` ((N - 20, N - 20) uint8 or uint16, as dicom.read_dicom_gray returns it), compared as
    vendor_to_u8 converts it. Row 0 then gains "reference" (the unaltered result vs the vendor image: the reference's m_sim_ovd), every
    other row "reference" (the altered result vs the vendor image) and "registered_reference" (the registered crop vs the same crop of
    the vendor image, rotations: of the vendor image rotated as rotated_reference rotates; None exactly where "registered" is None).
    On the device the vendor image sits in slot 2 (musica_sim_set_vendor_reference), rotated in slot 3, and its queries join the
    row's own launch. Without it the rows are exactly as before.

    symmetries: elements of the square's symmetry group (apply_symmetry; SYMMETRIES for the seven non-trivial ones). None or empty adds
    nothing. Otherwise rows d4_<e> follow the pn_* rows: the raw image under element e (on the device: alter_symmetry), "direct" against
    the unaltered result, "registered" over the WHOLE frame against the unaltered result under the same element, which an exactly
    equivariant pipeline would reproduce bit for bit. On the device that reference goes into slot 1 and the transformed vendor image into
    slot 3 (musica_sim_transform_reference; the rotation rows are done with them by then). These rows draw nothing from `rng` and do not
    advance the noise ordinal.

    tone: every comparison dict of a row gains a sibling with the five JOINT_METRICS (tone_similarities): direct_tone, registered_tone
    and, with a vendor image, reference_tone and registered_reference_tone; present exactly where the original is and None exactly
    where it is None. On the device the row's queries go through musica_sim_joint in one call, each comparison's tone_lut remaps its
    slot into one of the slots SLOT_TONE .. SLOT_TONE + 3 (musica_sim_remap_reference), and tone_ssim is musica_sim_compare's ssim
    against those slots over the same regions, one call per row. Without it the rows and the launches are exactly as before.

    displacement: a radius R > 0 measures where the output went by exact block matching (displacement_table). Every row gains
    "direct_shift": the full frame inset by R on every side against the unaltered result; rows with a registered comparison gain
    "registered_shift": that comparison's region inset by R against what it is compared with (None exactly where "registered" is None or
    the inset region has a side under 7). Each is a dict of SHIFT_KEYS (displacement_summary): (0, 0) in a registered row says the
    output moved as the input did. On the device the row's one or two queries go through one musica_sim_displace call; on the host the
    restatement runs on the same planes; both summarise exact integer tables with one function, so the two agree to the last bit.
    displacement_tiles: each *_shift dict also carries "tile_tables" ((tiles_y, tiles_x, S, S) uint32) and "size" ((w, h) of its
    region), what displacement_maps draws. With displacement=0 the rows and the launches are exactly as before.

    scales: S > 0 (at most SIM_MAX_SCALES) says at which spatial scale the output changed (multiscale_similarities). Every comparison
    dict of a row gains a sibling: direct_scales, registered_scales and, with a vendor image, reference_scales and
    registered_reference_scales; present exactly where the original is and None exactly where it is None. Each is a dict of SCALES_KEYS:
    ms_ssim, scales and the lists ssim, cs, lum, mse of length `scales`, a comparison using min(S, max_scales of its region). On the
    device the row's queries go through one musica_sim_multiscale call per distinct scale count; on the host the restatement scores
    the same crops. With scales=0 the rows and the launches are exactly as before.

    gradients: True compares what MUSICA amplifies, the edges of the image itself (gradient_statistics). Every comparison dict of a
    row gains a sibling: direct_gradient, registered_gradient and, with a vendor image, reference_gradient and
    registered_reference_gradient; present exactly where the original is and None exactly where it is None. Each is gradient_row's
    dict: the GRADIENT_KEYS gsim, gc, gain, turn, reversed, rmse and compression, gain_by_class (22 entries, None for an empty class)
    and "table", the exact 22 x 6 integers of the comparison's interior by the edge strength of its reference side. On the device the
    row's queries go through one musica_sim_gradients call behind the scales'; on the host the restatement scores the same crops.
    The integers are equal on every path and summarised by one function; gsim agrees to rounding (the device sums in its own fixed
    order). Anything but a bool is a ValueError; with gradients=False the rows and the launches are exactly as before.

    order: True asks whether the local order of the gray levels survived: is the same pixel still the darker one of a neighbouring
    pair (order_statistics: the census signs of both sides over the 7 x 7 neighbourhood). A monotone change of the gray levels, even a
    spatially varying one that stays locally monotone, scores as nothing; rebound rings, halos, reversed weak edges and flattened
    texture break orders. Every comparison dict of a row gains a sibling behind the gradient keys and before direct_reach: direct_order,
    registered_order and, with a vendor image, reference_order and registered_reference_order; present exactly where the original is
    and None exactly where it is None. Each is order_row's dict: the ORDER_KEYS tau, tau_by_ring (three entries), reversed, flattened,
    split, intact, distance, median and p95, "rings", the exact 3 x 5 integers per ring (pairs, same, reversed, flattened, split), and
    "histogram", the 97 numbers of interior pixels per census distance. On the device the row's queries go through one
    musica_sim_order call behind the gradients'; on the host the restatement scores the same crops. There is no float on the device:
    the integers are equal on every path and summarised by one function, so the rows are identical. Anything but a bool is a
    ValueError; with order=False the rows and the launches are exactly as before.

    ensemble: K > 0 (at most SIM_ENSEMBLE_MAX; needs runner.device_alterations, else ValueError) repeats every noise alteration K times and
    splits the change of the output into bias and noise (ensemble_statistics). Every row gains "ensemble": None for rows without noise,
    for c_sh_*, gn_* and pn_* a dict of "direct" (the full frame against the unaltered result, ENSEMBLE_KEYS), "registered" (the
    collimator's region; present exactly where the row's "registered" is, else None), "realisations" (K) and "per_realisation": "mean"
    and "std" (ddof = 1, 0 for K = 1) over the K realisations of the five SIM_METRICS of the direct comparison. The row's own keys and
    launches are untouched: the ensemble runs after the row is complete on a second context owned by the runner
    (runner.ensemble_context, batch runner.ensemble_batch) that holds the raw image as its source and the unaltered result in its slot 0.
    Realisation j of the row with ordinal o draws from the study's seed and the stream ensemble_stream(o, j); B realisations go through
    one step, musica_sim_ensemble_add and one musica_sim_compare call, and one musica_sim_ensemble_result call ends the row.
    ensemble_tiles: the "direct" dict also carries "tile_tables" ((tiles_y, tiles_x, 2) uint64) and "size", what ensemble_maps draws.
    With ensemble=0 nothing is created and the rows are exactly as before.

    covariance: a radius R > 0 (at most SIM_MAX_RADIUS; needs ensemble > 0, else ValueError) adds the texture of the noise: each noise
    row's "ensemble" dict gains "covariance": {"direct": ..., "registered": ...}, each a dict of COV_KEYS plus "nps_radial" and
    "hf_fraction" (covariance_row). The direct region is the full frame inset by R; the registered one the row's registered region inset
    by R, None where the row has none or an inset side is under 7. One musica_sim_ensemble_track call follows the row's reset and one
    musica_sim_ensemble_covariance call ends it. covariance_tiles: the dicts also carry "table" and "tile_tables". With covariance=0 the
    rows, keys and launches are exactly as before.

    blurs: radii of the resolution-loss rows (binomial_blur; BLURS for 1, 2, 4, 8), each in 1 .. BLUR_MAX_RADIUS, else ValueError before
    any work. None or empty adds nothing. Otherwise rows blur_<r> follow the d4_* rows: the raw image blurred with radius r (on the
    device: alter_blur), "direct" against the unaltered result (how much of the input's resolution loss reaches the output),
    "registered" over the frame inset by r (roi_blur) against the unaltered result blurred with the same radius (what a linear,
    shift-invariant processor would not show; None when the inset frame has a side under 8). On the device that reference goes into
    slot 1 and the blurred vendor image into slot 3 (musica_sim_blur_reference). Like the d4 rows they draw nothing from `rng` and take
    no ordinal; vendor, tone, scales and displacement apply to them as to a d4 row.

    zooms: magnifications (p, q) of the scale rows (zoom; ZOOMS for 1.05, 1.1, 1.25, 1.5 and 2), each 1 <= q < p <= ZOOM_MAX_P in lowest
    terms, else ValueError before any work. None or empty adds nothing. Otherwise rows zoom_<p>_<q> follow the blur_* rows: the raw image
    magnified by p / q about its centre (on the device: alter_zoom), "direct" against the unaltered result, "registered" over the WHOLE
    frame (roi_zoom: no fill, nothing to crop) against the unaltered result magnified alike, which a processor that commutes with
    magnification would reproduce. On the device that reference goes into slot 1 and the magnified vendor image into slot 3
    (musica_sim_zoom_reference). They draw nothing from `rng` and take no ordinal; vendor, tone, scales and displacement apply to them
    as to a d4 row.

    scatters: veils (R, a, b) of the scatter rows (scatter; SCATTERS(n) for the fractions 1/10, 1/4, 1/2, 2/3 and 4/5 at the radius of
    the image size), each 1 <= R <= SCATTER_MAX_RADIUS and 1 <= a < b <= SCATTER_MAX_DEN in lowest terms, else ValueError before any
    work. None or empty adds nothing. Otherwise rows scatter_<R>_<a>_<b> follow the zoom_* rows: the raw image mixed with its tent x
    tent blur of box radius R at the scatter fraction a / b (on the device: alter_scatter), "direct" against the unaltered result,
    "registered" over the frame inset by 2R (roi_scatter) against the unaltered result veiled alike: blur's registered comparison
    carried to low frequencies, what a linear, shift-invariant processor would not show (None when the inset frame has a side under
    8). On the device that reference goes into slot 1 and the veiled vendor image into slot 3 (musica_sim_scatter_reference). They draw
    nothing from `rng` and take no ordinal; vendor, tone, scales and displacement apply to them as to a d4 row.

    details: contrast-detail grids, each a detail list (x, y, r, c) for the raw plane (processing.detail_list; DETAILS(n) for the five
    contrasts 0.8 % .. 12.5 % on detail_grid's phantom) that is also valid for the output plane when shifted by the margin
    (output_details), else ValueError before any work. None adds nothing. Otherwise rows cd_<c> (c: the grid's first contrast) follow
    the scatter_* and warp rows: the raw image with the grid's discs inserted (insert_details; on the device: alter_details),
    "direct" scored as for every row, "registered" None (nothing moved, as for the noise rows), and every row of the study gains "details": None
    except in the cd_ rows, where it is detail_row's dict of the details measured where they lie against the unaltered result
    (detail_statistics; on the device one musica_sim_details call behind the row's musica_sim_compare, whose exact sq_diff_sum of the
    full frame gives outside_mse): per radius the count and the mean, min, max and population std over the positions of contrast,
    cnr, rose and halo, and outside_mse. Host and device summarise exact integers with one function, so "details" is equal to the
    last bit on every path. detail_tables: the dict also carries "per_detail". The rows draw nothing from `rng` and take no ordinal;
    vendor, tone, scales and displacement apply to "direct" as elsewhere. Nothing is asserted about visibility: these are findings.
    Three relations read off a cd_ study: locality (outside_mse near 0), monotonicity (more c, more contrast, at every radius) and
    position invariance (a small std over the positions); where MUSICA's local gains break the last one is the finding.

    edges: slanted-edge grids, each an edge list (x, y, h, p, q, o, c) for the raw plane (processing.edge_list; EDGES(n) for the five
    contrasts 0.8 % .. 12.5 % on edge_grid's phantom) that is also valid for the output plane when shifted by the margin
    (output_edges), else ValueError before any work. None adds nothing. Otherwise rows edge_<c> (c: the grid's first contrast) follow
    the cd_ rows: the raw image with the grid's plates inserted (insert_edges; on the device: alter_edges), "direct" scored as for
    every row, "registered" None, and every row of the study gains "edges": None except in the edge_ rows, where it is edge_row's dict
    of the edges measured where they lie against the unaltered result (edge_statistics; on the device one musica_sim_edges call behind
    the row's musica_sim_compare, whose exact sq_diff_sum of the full frame gives outside_mse): over all edges, per orientation and
    per half-side the min, mean, max and count of the step, the 10-90 % rise, the overshoot and undershoot, mtf50 and mtf_peak of
    the a - b edge-spread function (edge_summary), and outside_mse. Host and device summarise exact integers with one function, so
    "edges" is equal to the last bit on every path. edge_tables: the dict also carries "per_edge", the three edge-spread functions
    of every edge included. The rows draw nothing from `rng` and take no ordinal. Nothing is asserted about how an edge is rendered:
    these are findings. A linear, shift-invariant processor would give the same normalised response at every contrast, position,
    orientation and polarity; where MUSICA does not is the finding.

    gratings: grating grids, each a grating list (x, y, h, ux, uy, T, wave) for the raw plane (processing.grating_list; GRATINGS(n) for
    the five contrasts 0.8 % .. 12.5 % on grating_grid's phantom) that is also valid for the output plane when shifted by the margin
    (output_gratings), else ValueError before any work. None adds nothing. Otherwise rows grating_<c> (c: the largest |w| of the grid's
    first wave) follow the edge_ rows: the raw image with the grid's plates inserted (insert_gratings; on the device: alter_gratings),
    "direct" scored as for every row, "registered" None, and every row of the study gains "gratings": None except in the grating_
    rows, where it is grating_row's dict of the gratings measured where they lie against the unaltered result (grating_statistics; on
    the device one musica_sim_gratings call behind the row's musica_sim_compare, whose exact sq_diff_sum of the full frame gives
    outside_mse): over all gratings, per direction and per period the median, min, max and count of the gain, the harmonic distortion
    and the response of the a - b profile folded over one period (grating_summary), and outside_mse. Host and device summarise exact
    integers with one function, so "gratings" is equal to the last bit on every path. grating_tables: the dict also carries
    "per_grating", the folded profiles of every grating included. The rows draw nothing from `rng` and take no ordinal. Nothing is
    asserted about the gains: these are findings. A linear processor would give the same gain at every contrast and no harmonics;
    how MUSICA's gain falls with the amplitude and rises with the frequency, and what it adds at 2f and 3f, is the finding.

    gains: gain specs (name, gx, gy), the tables of a separable gain map for the raw plane's columns and rows in 1 / 4096
    (processing.gain_tables; GAINS(n) for the five exposures and the heel, vignette, band and line maps at the five strengths), else
    ValueError before any work. None adds nothing. Otherwise rows named by the specs follow the grating_ rows: the raw image under the
    map (apply_gain; on the device: alter_gain), "direct" scored as for every row, "registered" None (a normalising processor is
    expected to be invariant, which "direct" scores), and every row of the study gains "profiles": None except in the gain rows, where
    it is profile_row's dict of the exact column and row profiles of the result against the unaltered result over the full output
    frame (profile_statistics; on the device one musica_sim_profiles call behind the row's musica_sim_compare) with the map sliced into
    the output plane (output_gain): per axis the mean shift, the transfer (the slope of the lines' mean change on their relative
    gain), its correlation and residual, the peak, the line noise, the peak's visibility and the spread (profile_summary). Host and
    device summarise exact integers with one function, so "profiles" is equal to the last bit on every path. gain_tables: the dict
    also carries "tables" and "gains", the raw integers. The rows draw nothing from `rng` and take no ordinal. Nothing is asserted:
    these are findings. A processor that normalises would show no transfer at all; what survives of a line far below the pixel noise,
    and how far it spreads, is the finding.

    luts: tone-table specs (name, lut), each lut 65536 integers in 0 .. 65535 (processing.lut_table; LUTS(raw) for the 21 pedestals,
    saturations, coarser ADCs, gammas and the negative of the plane's own range), else ValueError before any work. None adds nothing.
    Otherwise rows named by the specs follow the gain rows: the raw image mapped point-wise through the table (apply_lut; on the device:
    alter_lut), "direct" scored as for every row, "registered" None (a processor that normalises and builds its tone curve from the
    histogram is expected to absorb a monotone table, which "direct" scores), and every row of the study gains "levels": None except
    in the lut rows, where it is level_row's dict of the exact sums of the result against the unaltered result over the full output
    frame per class of the unaltered input, raw >> level_shift(raw) under the output pixel (level_statistics with level_classes; on the
    device one musica_sim_levels call behind the row's musica_sim_compare, whose sq_diff_sum and pixels the table must add up to; with
    device_metrics alone the raw plane is made resident once for it): how many classes are occupied, the rms and largest shift of the
    characteristic curve, the slope and correlation of the new curve on the old, the share of the change that is a function of the
    input level alone, the within-class remainder, the ratio of the within-class scatters and the reversals (level_summary). Host and
    device summarise exact integers with one function, so "levels" is equal to the last bit on every path. lut_tables: the dict also
    carries "levels", "curve_a" and "curve_b", the two curves. The rows draw nothing from `rng` and take no ordinal. Nothing is asserted:
    these are findings. A processor that fully normalises would show no curve shift for any monotone table; what it makes of a coarser
    ADC, of saturation and of a negative is the finding.

    warps: local-deformation specs (name, field), each field an (M, M, 2) array of node displacements in 1 / 256 pixel on the 64-pixel
    control grid of the raw plane (warp; processing.warp_field; WARPS(n) for shifts, stretches, shears, bulges and twists of 0.25 to
    16 pixels), valid for the raw plane at origin 0 and for the output plane at the margin, else ValueError before any work. None or
    empty adds nothing. Otherwise rows named by the specs follow the scatter_* rows: the raw image warped by the field (on the device:
    alter_warp). "direct" against the unaltered result says how much of the deformation reaches the output; "registered", over the
    frame inset by the field's reach (roi_warp; None when the inset frame has a side under 8) against the unaltered result warped by
    the same field at the output plane's origin, says what a processor that commutes with the deformation would not show. On the
    device that reference goes into slot 1 and the warped vendor image into slot 3 (musica_sim_warp_reference). The rows draw nothing
    from `rng` and take no ordinal; vendor, tone, scales and displacement apply to them as to a zoom row. Every row of such a study
    gains "warp": None except in the warp rows, where it is {"reach": warp_reach(field), "peak": the largest |d| in pixels,
    "tracking"}; "tracking" is None without a displacement radius (or where the inset frame is too small) and else warp_tracking's
    dict from the tile tables of the row's DIRECT displacement comparison: how many 64 x 64 tiles there are, how many of their
    expected shifts the radius reaches, how many of those the block matching found, and the rms distance between measured and
    expected shift. Host and device tables are equal integers, so the dict is equal on every path. Nothing is asserted about the
    values: whether MUSICA's local gains let the output follow a deformation tile by tile is the finding.

    points: point-response grids, each a point list (x, y, R, s, c, group) for the raw plane (processing.point_list; POINTS(n) for a
    dead, a half-dead, a faint, a doubled and a hot element on point_grid's phantom) that is also valid for the output plane when
    shifted by the margin (output_points), else ValueError before any work. None adds nothing. Otherwise rows point_<c> (c: the grid's
    first contrast) follow every other row: the raw image with the grid's clusters altered (insert_points; on the device:
    alter_points; a dead element writes zeros into the input, which the noise and gradation histograms treat specially), "direct"
    scored as for every row, "registered" None, and every row of the study gains "points": None except in the point_ rows, where it is
    point_row's dict of the response stacked around the points against the unaltered result (point_statistics; on the device one
    musica_sim_points call behind the row's musica_sim_compare, whose exact sq_diff_sum of the full frame gives outside_mse): per
    group (cluster size) and over all points the peak, gain, volume, radial profile, fwhm, rebound, reach, anisotropy, spread and the
    dependence on the local background (point_summary), and outside_mse. Host and device summarise exact integers with one function,
    so "points" is equal to the last bit on every path. point_tables: the dict also carries "per_point" and "stacks". The rows draw
    nothing from `rng` and take no ordinal. Nothing is asserted: the narrow core, the wide skirt and the rebound ring of a multi-scale
    amplifier, and how they differ between a dead, a faint and a hot element, are the finding.

    reach: None (the default: the rows and the calls are exactly as without it), True for REACH_RADII(n), or a list of radii
    (processing.reach_radii: from 0, strictly ascending, at most 32 of at most 16383), else ValueError before any work. Every row gains
    "direct_reach" behind its gradient keys: None in the unaltered row and in a row whose alteration changed no pixel of the input or
    every one, else reach_row's dict of the row's DIRECT comparison over the full output frame, its exact sums kept apart by the
    Chebyshev distance of the pixel from the nearest changed input pixel (reach_classes, reach_statistics; on the device one
    musica_sim_reach call behind the row's musica_sim_compare, whose sq_diff_sum and pixels the table must add up to; with
    device_metrics alone the raw plane is made resident once for it): per class rmse, changed share, mean shift and max, and the
    extent beyond which nothing changed, the floor that no distance removes (the global stages), the spill out of the altered set,
    the radius of half the spill and the decay slope (reach_summary). Host and device summarise exact integers with one function, so
    the dict is equal to the last bit on every path. reach_tables: the dict also carries "table". reach_maps: it also carries "class_plane",
    the (N - 20)^2 classes of the output's pixels (on the device one musica_sim_reach_classes call more), what write_reach_maps draws. Nothing is asserted: how far the
    pyramid carries a local change, and how much of it the global stages spread over the whole frame, are the finding.

    observer: True (needs details, else ValueError; anything but a bool is one too) puts a model observer on the cd_ rows: a channelized
    Hotelling observer with Laguerre-Gauss channels (laguerre_gauss_bank, observer_summary). Every row of the study gains "observer"
    behind the relations' keys: None except in the cd_ rows, where it is observer_row's dict of the details' windows against the
    unaltered result at the details' output positions, one bank per distinct radius (observer_views; channel_responses, on the device
    one musica_sim_observer call behind the row's musica_sim_details): per radius the count, the detectability cho with its auc, the
    non-prewhitening npw on the disc channel, the spread of the Hotelling scores over the positions and the channels' snr. Every grid's
    radii must give banks the call takes (r <= 32, at most OBSERVER_MAX_BANKS distinct), else ValueError before any work. Host and
    device summarise exact integers with one function, so "observer" is equal to the last bit on every path; observer_curve reads the
    threshold contrast per radius off the cd_ rows. Nothing is asserted: these are findings. With observer=False the rows, keys and
    launches are exactly as before.

    codecs: DC steps of the lossy-compression rows (block_codec with codec_table(s); CODECS for 16, 64, 256, 1024, 4096), each in
    1 .. 65535, else ValueError before any work. None or empty adds nothing. Otherwise rows codec_<s> follow the warp rows: the raw image
    through the exact 8 x 8 block codec (on the device: alter_codec), "direct" against the unaltered result (how much of the codec's loss
    reaches the output), "registered" over the whole output frame against the unaltered result compressed alike: the 8-bit plane through
    block_codec with codec_table8 of the same table at the origin PROCESSING_MARGIN % 8, so its blocks lie where the raw plane's lay
    (on the device: musica_sim_codec_reference into slot 1, the vendor image into slot 3). That is compress-before against
    compress-after. Like the blur rows they draw nothing from `rng` and take no ordinal; every metric of the study applies to them.

    lattice: a period P in LATTICE_PERIODS asks how much of every change sits on a lattice of the raw grid (lattice_statistics: a
    comparison's sums folded by the position modulo P, at the origin PROCESSING_MARGIN % P, the raw plane's lattice seen from the output
    plane): the 8 x 8 blocks of a codec row, and the decimated pyramid's own periods 2 .. 32 in the t_x_, shift_ and zoom_ rows. Every
    comparison dict of a row gains a sibling behind all other keys: direct_lattice, registered_lattice and, with a vendor image,
    reference_lattice and registered_reference_lattice; present exactly where the original is and None exactly where it is None. Each
    is lattice_row's dict: per axis "x" and "y" the LATTICE_AXIS_KEYS step_a, step_b, amplified and phase_mse, then "periodic" and the
    exact "table" (lattice_summary). On the device one musica_sim_lattice call behind the order's; on the host the restatement scores
    the same crops. There is no float on the device and one summary function: the values are equal to the last bit on every path.
    Anything but 0 or one of the five periods is a ValueError; with lattice=0 the rows and the launches are exactly as before. Nothing
    asserts how much the pipeline amplifies blocking: that is the finding.

    blobs: a threshold T in 0 .. 254 (processing.blob_threshold; None: off) asks whether the changed pixels of every comparison form
    objects: the connected components (blob_connectivity: 4 or 8) of the mask |a - b| > T (blob_statistics). Every comparison dict of a
    row gains a sibling behind all other keys, the lattice's included: direct_blobs, registered_blobs and, with a vendor image,
    reference_blobs and registered_reference_blobs; present exactly where the original is and None exactly where it is None. Each is
    blob_row's dict: blob_summary's BLOB_KEYS (the components, the changed, isolated, clustered and largest shares, the mean size, the
    fill and the border share), "largest_box", the per-class "class_components" and "class_pixels" and the exact "table". On the device
    one musica_sim_blobs call behind the lattice's; on the host the restatement labels the same crops. Everything is an integer and
    there is one summary function: the values are equal to the last bit on every path. With blobs=None the rows and the launches are
    exactly as before. Label maps are not written.

    spectrum: a tile side T, one of 8, 16, 32, 64 (processing.spectrum_tile; None: off), asks which spatial frequency band and
    orientation of the image itself every comparison changed, and by what gain: the exact Walsh-Hadamard transforms of the whole T x T
    tiles of both sides (spectrum_statistics; the Walsh octaves are the Haar subbands). Every comparison dict of a row gains a sibling
    behind all other keys, the blobs' included: direct_spectrum, registered_spectrum and, with a vendor image, reference_spectrum and
    registered_reference_spectrum; present exactly where the original is, None where it is None or where its region holds no whole
    tile. Each is spectrum_row's dict: spectrum_summary's "bands" and "radial" (gain, coherence and error share per band pair and per
    radial band), the SPECTRUM_KEYS (slope, the horizontal, vertical, diagonal and dc error shares, ac_gain, ac_coherence), "tile",
    "tiles" and the exact "table". On the device one musica_sim_spectrum call behind the blobs'; on the host the restatement
    transforms the same crops. Everything is an integer and there is one summary function: the values are equal to the last bit on
    every path. Anything but None or one of the four sides is a ValueError; with spectrum=None the rows and the launches are exactly as
    before. Nothing asserts what the gains are: that is the finding.

    texture: the gray levels G, one of 8, 16, 32, 64 (processing.cooccurrence_levels; None: off), asks whether the texture of the image
    survived: the gray-level co-occurrence matrices (Haralick 1973) of both sides of every comparison at texture_distances (1 .. 4
    distinct ascending distances 1 .. 16, processing.cooccurrence_distances; checked like blob_connectivity, whether texture is given
    or not) in the directions 0, 45, 90, 135 degrees (cooccurrence_statistics). Every comparison dict of a row gains a sibling behind
    all other keys, the spectrum's included: direct_texture, registered_texture and, with a vendor image, reference_texture and
    registered_reference_texture; present exactly where the original is, None where it is None or where its region has no pair at any
    distance. Each is texture_row's dict: cooccurrence_summary's "distances" (per distance contrast, dissimilarity, homogeneity,
    energy, entropy, correlation and anisotropy of either side, their differences and the Jensen-Shannon divergence; None for a
    distance without a pair) and the largest "divergence", "levels", "distance_list" and the exact "pairs". On the device one
    musica_sim_cooccurrence call behind the spectrum's; on the host the restatement counts the same crops. The tables are integers
    and there is one summary function: the values are equal to the last bit on every path. With texture=None the rows and the launches
    are exactly as before.

    granulometry: a radii list, 1 .. 8 distinct ascending integers 1 .. 16 (processing.granulometry_radii; None: off), asks which object
    sizes became brighter or darker: the openings and closings of both sides of every comparison by the growing (2 r + 1)^2 square,
    clipped to the region (granulometry_statistics). Every comparison dict of a row gains a sibling behind all other keys, the
    texture's included: direct_granulometry, registered_granulometry and, with a vendor image, reference_granulometry and
    registered_reference_granulometry; present exactly where the original is, None where it is None. Each is granulometry_row's dict:
    granulometry_summary's "bright" and "dark" (per class the pattern-spectrum shares of either side, gain, coherence and mse; the mean
    element sides and their shift, the slope of log gain on log side, the residue's shift), "radii", "pixels" and the exact "table". On
    the device one musica_sim_granulometry call behind the texture's; on the host the restatement sieves the same crops. The tables
    are integers and there is one summary function: the values are equal to the last bit on every path. With granulometry=None the
    rows and the launches are exactly as before.

    contours: a threshold tau on the squared Sobel gradient, an integer 1 .. 1 300 500 (processing.contour_threshold; None: off), asks
    whether the contours of the output are where the contours of the reference are: both sides' thinned edge sets and, per contour pixel
    of one side, the exact squared distance to the nearest contour pixel of the other, resolved up to contour_radius, 1 .. 32
    (processing.contour_radius; contour_statistics). Every comparison dict of a row gains a sibling behind all other keys, the
    granulometry's included: direct_contours, registered_contours and, with a vendor image, reference_contours and
    registered_reference_contours; present exactly where the original is, None where it is None. Each is contour_row's dict:
    contour_summary's sizes, densities and ratio of the two sets, Pratt's figure of merit "fom", the "kept", "moved" and "lost" shares
    of the reference's contour, the "spurious" share of the output's, per direction the mean, median and 95th percentile of the
    distance, the "hausdorff" distance, then "threshold", "radius", "pixels" and the exact "table"; with contour_maps also "planes",
    the byte plane (bit 0: the output's contour, bit 1: the reference's) that report.write_contour_maps draws. On the device one
    musica_sim_contours call behind the granulometry's; on the host the restatement takes the same crops. The tables are integers and
    there is one summary function: the values are equal to the last bit on every path. With contours=None the rows and the launches
    are exactly as before.

    minkowski: a flag (anything but a bool is refused) asks what the gray-level landscape of the output looks like as a shape: the three
    Minkowski functionals, area, perimeter and Euler characteristic, of every threshold set {v >= t} of the output, of the reference
    and of their pixel-wise minimum, from eight exact cell histograms a side (minkowski_statistics). Every comparison dict of a row
    gains a sibling behind all other keys, the contours' included: direct_minkowski, registered_minkowski and, with a vendor image,
    reference_minkowski and registered_reference_minkowski; present exactly where the original is, None where it is None. Each is
    minkowski_row's dict: minkowski_summary's "pixels", per side the mean, the total variation "tv", the most "islands" and "holes"
    with their levels and the outline "contact", "tv_gain", the normalised L1 distances of the four curves, the "overlap" of the upper
    sets with its smallest level, the tone-free "matched" read-out at the area fractions 1 / 8 .. 7 / 8 with its two distances, which
    no increasing tone curve changes, and the exact "table"; with minkowski_curves (a flag) also "curves", the (3, 5, 256) array that
    report.write_minkowski_curves writes. On the device one musica_sim_minkowski call behind the contours'; on the host the
    restatement takes the same crops. The tables are integers and there is one summary function: the values are equal to the last bit
    on every path. With minkowski=False the rows and the launches are exactly as before."""
    options = {k: v for k, v in locals().items() if k not in ("raw", "runner", "rng")}   # every option by its name, as study_options takes them
    rng = rng or np.random.default_rng(0)
    opt = study_options(raw.shape[0], runner, **options)
    unalt = runner.run(raw)
    shape = unalt.shape
    full = (0, 0, 0, 0, shape[1], shape[0])
    scorer = (DeviceScorer if getattr(runner, "device_metrics", False) else HostScorer)(runner, opt, unalt)   # the one place that asks
    scorer.source = raw   # what reach() takes the input's change against
    metrics = [("", scorer.similarities)] + [("_" + m.suffix, functools.partial(scorer.score, m)) for m in SCORED_METRICS if m.on(getattr(opt, m.option))]
    rows = []

    def row(alteration=None, eproc=None):
        """One row, the unaltered one without an alteration: the output produced, every comparison it has scored with every metric of
        the study, in the order compare, tone, scales, gradients, order, lattice, blobs, spectrum, texture, granulometry, contours, minkowski, displacement; then, with the ensemble's context, the row's ensemble."""
        registered = None   # (reference key, region) of the registered comparison
        if alteration is not None:
            scorer.produce(alteration)
            if alteration.move:
                scorer.move(*alteration.move)
            region = alteration.region() if alteration.region else None
            if region is not None and min(region[4], region[5]) >= 8:
                registered = (SLOT_ROTATED if alteration.move else SLOT_UNALTERED, region)
        own = [("direct", (SLOT_UNALTERED, full))] + ([("registered", registered)] if registered else [])
        compared = []   # (row key, comparison) in the queries' order: each of the row's own, then the same against the vendor image
        for key, (slot, region) in own:
            compared.append((key, (slot, region)))
            if opt.vendor is not None:
                compared.append((VENDOR_KEY[key], (VENDOR_SLOT[slot], region)))
        out = dict.fromkeys(k for k in opt.keys if alteration is not None or not k.startswith("registered_reference"))
        out["alteration"] = alteration.name if alteration is not None else "unaltered"
        for suffix, score in metrics:
            out.update(zip([key + suffix for key, _ in compared], score([c for _, c in compared])))
        if opt.reach is not None and alteration is not None:   # behind the row's comparisons: the direct one's integers are checked against
            out["direct_reach"], = scorer.reach([(SLOT_UNALTERED, full)])
        if opt.displacement:   # a *_shift stays None without its comparison, or where the inset leaves a side under 7
            shifted = [(key + "_shift", (slot, _inset(region, opt.displacement))) for key, (slot, region) in own]
            shifted = [(key, c) for key, c in shifted if c[1] is not None]
            tracked = alteration is not None and alteration.warp is not None   # a warp row reads its direct comparison's tile tables
            out.update(zip([key for key, _ in shifted], scorer.shifts([c for _, c in shifted], keep=tracked)))
        if alteration is not None and alteration.warp is not None:
            direct = out.get("direct_shift")
            out["warp"] = {"reach": warp_reach(alteration.warp), "peak": int(np.abs(alteration.warp.astype(np.int64)).max()) / mp.WARP_UNIT,
                           "tracking": warp_tracking(alteration.warp, (PROCESSING_MARGIN,) * 2, _inset(full, opt.displacement), direct["tile_tables"])
                           if direct else None}
            if not opt.displacement_tiles:
                for key in ("direct_shift", "registered_shift"):
                    if out.get(key):
                        del out[key]["tile_tables"], out[key]["size"]
        if alteration is not None and alteration.measure:
            relation, payload = alteration.measure
            out[relation.key] = scorer.measure(relation, relation.output(payload))
            if opt.observer and relation.key == "details":
                out["observer"] = scorer.observer(relation.output(payload))
        out["mean_cnr"] = runner.mean_cnr() if runner.proc else None
        if eproc is not None:
            out["ensemble"] = ensemble_of(eproc, alteration.noise, registered[1] if registered else None, full, opt)
        rows.append(out)

    row()
    seed = eproc = None
    if opt.device_alterations:
        runner.proc.alter_set_source(raw)
        seed = int(rng.integers(0, 2 ** 63))
    elif (opt.luts or opt.reach is not None) and getattr(runner, "device_metrics", False):
        runner.proc.alter_set_source(raw)   # musica_sim_levels takes its classes from the resident source plane, musica_sim_reach the unchanged input
    if opt.ensemble:
        eproc = runner.ensemble_context(opt.ensemble)
        eproc.alter_set_source(raw)
        for i in range(eproc.batch):     # every image of the batch holds a valid input, whatever the last chunk leaves unused
            eproc.alter_none(i)
        eproc.sim_set_reference(SLOT_UNALTERED, runner.proc.sim_get_reference(SLOT_UNALTERED))
    for alteration in study_alterations(raw, rng, runner.proc, seed, shape, opt):
        row(alteration, eproc)
    return rows


def read_manifest(path):
    """The images of a --manifest file: one `raw[,reference]` per line, `#` starts a comment, blank lines are skipped. Paths are
    relative to the manifest's directory (either slash separates directories, so the reference's `foot\\image.raw` works as written).
    Returns [(raw as written, raw path, reference path or None)]."""
    base = os.path.dirname(os.path.abspath(path))

    def resolve(p):
        return os.path.join(base, *[s for s in p.replace("\\", "/").split("/") if s]) if not os.path.isabs(p) else p

    entries = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            parts = [s.strip() for s in line.split(",")]
            if len(parts) > 2 or not all(parts):
                raise ValueError("%s:%d: expected `raw[,reference]`, got %r" % (path, ln, line))
            entries.append((parts[0], resolve(parts[0]), resolve(parts[1]) if len(parts) == 2 else None))
    if not entries:
        raise ValueError("%s: no images" % path)
    return entries


def run_studies(entries, runner, **study_args):
    """run_study over several raw images through one runner: `entries` as read_manifest returns them (raw paths of the runner's size;
    a reference: the vendor DICOM, read with dicom.read_dicom_gray). Every image gets a fresh np.random.default_rng(0), so its rows are
    those of a study of that image alone; luts=True stands for LUTS of each image. Returns [(raw as written, rows)], for write_studies_csvs."""
    from .dicom import read_dicom_gray
    from .processing import read_raw
    studies = []
    for name, raw_path, ref_path in entries:
        raw = read_raw(raw_path, runner.n)
        if raw is None:
            raise ValueError("%s: not a raw file of %d x %d pixels (256-byte header + N*N uint16)" % (raw_path, runner.n, runner.n))
        vendor = read_dicom_gray(ref_path) if ref_path else None
        per_image = dict(study_args, luts=LUTS(raw)) if study_args.get("luts") is True else study_args   # the tables follow each plane's own range
        studies.append((name, run_study(raw, runner, rng=np.random.default_rng(0), vendor=vendor, **per_image)))
    return studies


def _comma_list(text, parse, expected, detail=False, valid=None, refused=None):
    """What the comma-list flags share: parse(the parts) gives the values; ArgumentTypeError(expected) where it raises ValueError
    (detail: followed by the error's own text), ArgumentTypeError(refused) where a value is not valid()."""
    import argparse
    try:
        values = tuple(parse(text.split(",")))
    except ValueError as e:
        raise argparse.ArgumentTypeError(expected + (": %s" % e if detail and str(e) else ""))
    if valid is not None and (not values or any(not valid(v) for v in values)):
        raise argparse.ArgumentTypeError(refused)
    return values


def _ints(parts):
    return [int(t) for t in parts]


def symmetry_list(text):
    """--symmetries' comma list of elements 0 .. 7."""
    return _comma_list(text, _ints, "expected a comma-separated list of elements 0 .. 7, got %r" % text,
                       valid=lambda e: 0 <= e <= 7, refused="symmetry elements are 0 .. 7, got %r" % text)


def blur_list(text):
    """--blurs' comma list of radii 1 .. BLUR_MAX_RADIUS."""
    return _comma_list(text, _ints, "expected a comma-separated list of radii 1 .. %d, got %r" % (mp.BLUR_MAX_RADIUS, text),
                       valid=lambda r: 1 <= r <= mp.BLUR_MAX_RADIUS, refused="blur radii are 1 .. %d, got %r" % (mp.BLUR_MAX_RADIUS, text))


def zoom_list(text):
    """--zooms' comma list of magnifications P/Q: 1 <= Q < P <= ZOOM_MAX_P in lowest terms."""
    def ratios(parts):
        zooms = [tuple(int(v) for v in t.split("/")) for t in parts]
        if any(len(z) != 2 for z in zooms):
            raise ValueError
        return [mp.zoom_ratio(z) for z in zooms]
    return _comma_list(text, ratios, "expected a comma-separated list of magnifications P/Q (1 <= Q < P <= %d, lowest terms), got %r"
                       % (mp.ZOOM_MAX_P, text), detail=True)


def scatter_list(text):
    """--scatters' comma list of veils R:A/B: 1 <= R <= SCATTER_MAX_RADIUS, 1 <= A < B <= SCATTER_MAX_DEN in lowest terms."""
    def veils(parts):
        for t in parts:
            radius, fraction = t.split(":")
            a, b = fraction.split("/")
            yield mp.scatter_spec((int(radius), int(a), int(b)))
    return _comma_list(text, veils, "expected a comma-separated list of veils R:A/B (1 <= R <= %d, 1 <= A < B <= %d, lowest terms), got %r"
                       % (mp.SCATTER_MAX_RADIUS, mp.SCATTER_MAX_DEN, text), detail=True)


def warp_list(text):
    """--warps' comma list of names of WARPS: <family>_<amplitude>."""
    known = ["%s_%d" % (f, a) for f in ("shift", "stretch", "shear", "bulge", "twist") for a in WARP_AMPLITUDES]
    return _comma_list(text, tuple, None, valid=known.__contains__,
                       refused="expected a comma-separated list of warps out of %s, got %r" % (",".join(known), text))


def granulometry_list(text):
    """--granulometry r1,r2,...: radii 1 .. 16, distinct and ascending (processing.granulometry_radii)."""
    import argparse
    try:
        return mp.granulometry_radii([int(t) for t in text.split(",")])
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def contour_tau(text):
    """--contours TAU: the threshold on the squared Sobel gradient, 1 .. 1 300 500 (processing.contour_threshold)."""
    import argparse
    try:
        return mp.contour_threshold(int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def contour_reach(text):
    """--contour-radius R: 1 .. 32 (processing.contour_radius)."""
    import argparse
    try:
        return mp.contour_radius(int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def reach_list(text):
    """--reach R0,R1,...: radii from 0, strictly ascending (processing.reach_radii)."""
    import argparse
    try:
        return [int(v) for v in mp.reach_radii([int(t) for t in text.split(",")])]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def codec_list(text):
    """--codecs' comma list of DC steps 1 .. 65535."""
    return _comma_list(text, _ints, "expected a comma-separated list of DC steps 1 .. 65535, got %r" % (text,),
                       valid=lambda s: 1 <= s <= 65535, refused="codec DC steps are 1 .. 65535, got %r" % (text,))


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Metamorphic study of raw images (or a seeded phantom) on the HIP MUSICA path")
    ap.add_argument("--raw", help="raw file: 256-byte header + N*N little-endian uint16 (test/standalone/main.cpp:54-75)")
    ap.add_argument("--reference", help="the vendor-processed DICOM of --raw (or of the phantom): fills the \"vs reference\" columns and "
                                        "writes ref_similarities.csv (script.py:370-411)")
    ap.add_argument("--manifest", help="text file with one `raw[,reference]` per line (paths relative to it, # comments): every image "
                                       "through one runner into the same CSV files; excludes --raw and --reference")
    ap.add_argument("--phantom-seed", type=int, default=1, help="seed of the synthetic phantom used when --raw is absent")
    ap.add_argument("--size", type=int, default=3072, help="image side N (the reference's CLI fixes 3072)")
    ap.add_argument("--levels", type=int, default=0)
    ap.add_argument("--out", default="out", help="directory of the CSV files")
    ap.add_argument("--cli", action="store_true", help="run every image through the musica-standalone process (run_process, script.py:200-214)")
    ap.add_argument("--device-metrics", action="store_true", help="compute MSE, SSIM and the histogram distances on the GPU (musica_sim_compare)")
    ap.add_argument("--device-alterations", action="store_true",
                    help="generate the alterations on the GPU (musica_alter; implies --device-metrics); the noise rows then come from a "
                         "different, reproducible, random stream than the host study's")
    ap.add_argument("--symmetries", nargs="?", const=SYMMETRIES, default=None, type=symmetry_list, metavar="E,E,...",
                    help="add the rows d4_<e>: the raw image under elements of the square's symmetry group (1, 3: quarter turns, 2: half turn, "
                         "4: transpose, 5, 7: flips, 6: anti-transpose), compared over the whole frame; without a list, all seven")
    ap.add_argument("--blurs", nargs="?", const=BLURS, default=None, type=blur_list, metavar="R,R,...",
                    help="add the rows blur_<r>: the raw image under the exact binomial blur of radius r (1 .. 8; sigma = sqrt(r / 2) pixels), "
                         "compared directly and, inset by r, with the unaltered result blurred alike; without a list, 1,2,4,8")
    ap.add_argument("--zooms", nargs="?", const=ZOOMS, default=None, type=zoom_list, metavar="P/Q,P/Q,...",
                    help="add the rows zoom_<p>_<q>: the raw image magnified by P/Q about its centre (exact integer bilinear; 1 <= Q < P <= 32 "
                         "in lowest terms), compared directly and, over the whole frame, with the unaltered result magnified alike; without "
                         "a list, 21/20,11/10,5/4,3/2,2/1")
    ap.add_argument("--scatters", nargs="?", const=True, default=None, type=scatter_list, metavar="R:A/B,R:A/B,...",
                    help="add the rows scatter_<R>_<a>_<b>: the raw image under the exact veiling glare of scatter fraction A/B (1 <= A < B <= 64 "
                         "in lowest terms) and box radius R (1 .. 127; the tent x tent veil has sigma = sqrt(2R(R+1)/3) pixels), compared "
                         "directly and, inset by 2R, with the unaltered result veiled alike; without a list, 1/10,1/4,1/2,2/3,4/5 at "
                         "R = round(127 * size / 3072)")
    ap.add_argument("--warps", nargs="?", const=True, default=None, type=warp_list, metavar="NAME,NAME,...",
                    help="add the local-deformation rows (WARPS): shift, stretch, shear, bulge and twist fields on a 64-pixel control grid at "
                         "the amplitudes 64, 256, 1024, 2048, 4096 / 256 pixels, the raw image warped exactly (integer bilinear), compared "
                         "directly and, inset by the field's reach, with the unaltered result warped alike; with --displacement the tiles' "
                         "best shifts are scored against the field's, written to warp_response.csv; on the GPU with --device-alterations "
                         "(musica_alter_warp, musica_sim_warp_reference); without a list, all 25")
    ap.add_argument("--details", action="store_true",
                    help="add the rows cd_<c>: discs of radius 1 .. 32 inserted on a grid (detail_grid) at the contrasts c / 1024 = 0.8 %% .. "
                         "12.5 %%, measured where they lie (contrast, cnr, halo per radius; the change away from them), written to "
                         "contrast_detail.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_details, "
                         "musica_alter_details)")
    ap.add_argument("--detail-tables", action="store_true", help="with --details: keep every detail's numbers in the rows (\"per_detail\")")
    ap.add_argument("--edges", action="store_true",
                    help="add the rows edge_<c>: slanted-edge plates in all four orientations inserted on a grid (edge_grid) at the contrasts "
                         "c / 1024 = 0.8 %% .. 12.5 %%, their edge-spread functions measured where they lie (step, 10-90 %% rise, overshoot, "
                         "undershoot, edge MTF per orientation), written to edge_response.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_edges, musica_alter_edges)")
    ap.add_argument("--edge-tables", action="store_true", help="with --edges: keep every edge's numbers and edge-spread functions in the rows (\"per_edge\")")
    ap.add_argument("--gratings", action="store_true",
                    help="add the rows grating_<c>: cosine patches of the periods 2 .. 32 pixels in four directions inserted on a grid "
                         "(grating_grid) at the contrasts c / 1024 = 0.8 %% .. 12.5 %%, the output folded by phase where they lie (gain, "
                         "harmonic distortion and response per period), written to grating_response.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_gratings, musica_alter_gratings)")
    ap.add_argument("--grating-tables", action="store_true", help="with --gratings: keep every grating's numbers and folded profiles in the rows (\"per_grating\")")
    ap.add_argument("--gains", action="store_true",
                    help="add the detector-gain rows (GAINS): the exposures 1/4 .. 2, and a heel effect, a vignetting, gain bands and defective "
                         "lines at the strengths c / 1024 = 0.8 %% .. 12.5 %%, each a separable gain map; the exact row and column profiles "
                         "of the result against the unaltered one (transfer, peak, line noise, visibility, spread per axis), written to "
                         "gain_response.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_profiles, musica_alter_gain)")
    ap.add_argument("--gain-tables", action="store_true", help="with --gains: keep the profiles' integers and the gains in the rows (\"tables\", \"gains\")")
    ap.add_argument("--luts", action="store_true",
                    help="add the tone-table rows (LUTS): pedestals, saturations, coarser ADCs, gammas and the negative of the image's own range, "
                         "each a point-wise map of the raw gray levels; the exact sums of the result against the unaltered one per level of the "
                         "input (curve shift, slope, global fraction, within-class remainder, spread ratio, reversals), written to "
                         "level_response.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_levels, musica_alter_lut)")
    ap.add_argument("--lut-tables", action="store_true", help="with --luts: keep the two characteristic curves in the rows (\"levels\", \"curve_a\", \"curve_b\")")
    ap.add_argument("--points", action="store_true",
                    help="add the rows point_<c>: defect pixels and 2 x 2 and 3 x 3 clusters on a grid (point_grid), dead, half-dead, faint, "
                         "doubled and hot (c / 1024 = 1, 0.5, 0.0625, -1, -63), the two-dimensional response stacked around them (peak, gain, "
                         "fwhm, rebound, reach, anisotropy, spread; the change beyond the windows), written to point_response.csv; on the GPU "
                         "with --device-metrics / --device-alterations (musica_sim_points, musica_alter_points)")
    ap.add_argument("--point-tables", action="store_true", help="with --points: keep every point's sums and the stacks in the rows (\"per_point\", \"stacks\")")
    ap.add_argument("--tone", action="store_true",
                    help="add the joint-histogram tone metrics of every comparison (mutual information, correlation ratio, tone-matched mse and "
                         "ssim) and write them to tone_robustness.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_joint)")
    ap.add_argument("--displacement", type=int, default=0, metavar="R",
                    help="measure where the output went: exact block matching over all integer shifts within R (1 .. 16) pixels, per row the "
                         "direct and the registered comparison, written to displacement.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_displace)")
    ap.add_argument("--displacement-maps", metavar="DIR",
                    help="with --displacement: two 8-bit BMPs per registered row into DIR, one pixel per 64 x 64 tile: the tile RMSE at the zero "
                         "shift and the length of the tile's best shift")
    ap.add_argument("--scales", type=int, default=0, metavar="S",
                    help="say at which spatial scale the output changed: SSIM, its contrast-structure factor and mse at S (1 .. 5) scales of "
                         "2 x 2 pooling and their MS-SSIM product, per comparison, written to scale_robustness.csv; on the GPU with "
                         "--device-metrics / --device-alterations (musica_sim_multiscale)")
    ap.add_argument("--gradients", action="store_true",
                    help="compare what MUSICA amplifies, the edges of the image itself: the exact Sobel gradient sums of every comparison by "
                         "the edge strength of its reference side (gradient similarity and correlation, gain, turn, reversed share, rmse, "
                         "gain per class and its compression slope), written to gradient_robustness.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_gradients)")
    ap.add_argument("--codecs", nargs="?", const=CODECS, default=None, type=codec_list, metavar="S,S,...",
                    help="add the rows codec_<s>: the raw image through the exact 8 x 8 integer block codec with the JPEG luminance table "
                         "scaled to the DC step s (1 .. 65535), compared directly and with the unaltered result compressed alike "
                         "(compress-before against compress-after); without a list, 16,64,256,1024,4096")
    ap.add_argument("--lattice", type=int, default=0, choices=(0,) + LATTICE_PERIODS, metavar="P",
                    help="fold every comparison's sums by the position modulo P on the raw grid (2, 4, 8, 16 or 32): the steps across the "
                         "lattice lines, their amplification and the periodic share of the change, written to lattice_robustness.csv; on "
                         "the GPU with --device-metrics / --device-alterations (musica_sim_lattice)")
    ap.add_argument("--blobs", type=int, default=None, choices=range(255), metavar="T",
                    help="label the connected components of every comparison's change mask |a - b| > T (0 .. 254): how many there are, how "
                         "much of the change is isolated pixels and how much sits in components of 16 pixels or more, the largest one's "
                         "share and box, written to blob_robustness.csv; on the GPU with --device-metrics / --device-alterations "
                         "(musica_sim_blobs)")
    ap.add_argument("--spectrum", type=int, default=None, choices=mp.SPECTRUM_TILES, metavar="T",
                    help="add the exact Walsh spectrum of every comparison over its whole T x T tiles, T one of 8, 16, 32, 64: gain, coherence "
                         "and error share per octave band and orientation, written to spectrum_robustness.csv; on the GPU with "
                         "--device-metrics / --device-alterations (musica_sim_spectrum)")
    ap.add_argument("--texture", type=int, default=None, choices=mp.COOCCURRENCE_LEVELS, metavar="G",
                    help="add the texture of every comparison: the gray-level co-occurrence matrices of both sides at G levels, G one of 8, 16, "
                         "32, 64, and Haralick's contrast, dissimilarity, homogeneity, energy, entropy and correlation, the anisotropy and the "
                         "Jensen-Shannon divergence of the two sides per distance, written to texture_robustness.csv; on the GPU with "
                         "--device-metrics / --device-alterations (musica_sim_cooccurrence)")
    ap.add_argument("--texture-distances", type=lambda v: tuple(int(d) for d in v.split(",")), default=mp.COOCCURRENCE_DISTANCES, metavar="d0,d1,..",
                    help="the distances of --texture: 1 .. 4 distinct ascending integers 1 .. 16 (default 1,2,4,8)")
    ap.add_argument("--granulometry", nargs="?", const=mp.GRANULOMETRY_RADII, default=None, type=granulometry_list, metavar="r1,r2,..",
                    help="add the sizes of every comparison: the granulometry of both sides, openings and closings by the growing (2 r + 1)^2 "
                         "square at 1 .. 8 distinct ascending radii 1 .. 16 (without a list 1,2,4,8,16): per polarity and size class the "
                         "pattern-spectrum shares, gain, coherence and mse, the mean element side and the slope of log gain on log side, "
                         "written to granulometry_robustness.csv; on the GPU with --device-metrics / --device-alterations "
                         "(musica_sim_granulometry)")
    ap.add_argument("--contours", nargs="?", const=mp.CONTOURS_THRESHOLD, default=None, type=contour_tau, metavar="TAU",
                    help="add the contours of every comparison: the thinned Sobel edge sets of both sides (squared gradient >= TAU, 1 .. 1300500; "
                         "without a value 4096: |g| >= 64, a straight step of 16 of 255 gray levels) and the exact distances between them: "
                         "Pratt's figure of merit, the kept, moved, lost and spurious shares, mean, median and 95th percentile of the distance "
                         "and the Hausdorff distance, written to contour_robustness.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_contours)")
    ap.add_argument("--contour-radius", type=contour_reach, default=mp.CONTOURS_RADIUS, metavar="R",
                    help="the radius up to which --contours resolves a distance, 1 .. 32 (default 16): a contour pixel without a partner within R is lost or spurious")
    ap.add_argument("--contour-maps", metavar="DIR", default=None,
                    help="with --contours: draw the two contours of every registered row (the output's alone 85, the reference's alone 170, both 255) as BMPs into DIR")
    ap.add_argument("--minkowski", action="store_true",
                    help="add the shape of every comparison's level sets: the Minkowski functionals (area, perimeter, Euler characteristic) of every "
                         "threshold set of the output, of the reference and of their minimum, exact for all 255 levels: total variation, islands, "
                         "holes, the overlap of the upper sets and a read-out at matched area fractions that no increasing tone curve changes, "
                         "written to minkowski_robustness.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_minkowski)")
    ap.add_argument("--minkowski-curves", metavar="DIR", default=None,
                    help="with --minkowski: write the five curves of every row, comparison and side at the levels 1 .. 255 as one CSV a raw file into DIR")
    ap.add_argument("--blob-connectivity", type=int, default=8, choices=(4, 8), help="the neighbourhood of --blobs (default 8)")
    ap.add_argument("--order", action="store_true",
                    help="ask whether the local order of the gray levels survived: the census signs of every comparison over the 7 x 7 "
                         "neighbourhood (Kendall's tau of centre-neighbour pairs, overall and per ring, the reversed, flattened and split "
                         "shares, the intact share and the census distance), written to order_robustness.csv; on the GPU with "
                         "--device-metrics / --device-alterations (musica_sim_order)")
    ap.add_argument("--observer", action="store_true",
                    help="with --details: a model observer on the cd_ rows, a channelized Hotelling observer with six Laguerre-Gauss channels "
                         "and the disc as a non-prewhitening template (detectability, auc, position spread and channel snr per radius, and "
                         "the threshold contrast against radius), written to observer.csv; on the GPU with --device-metrics / "
                         "--device-alterations (musica_sim_observer)")
    ap.add_argument("--reach", nargs="?", const=True, default=None, type=reach_list, metavar="R0,R1,...",
                    help="keep every row's direct comparison apart by the Chebyshev distance from the nearest changed input pixel: rmse, changed "
                         "share, shift and max per distance class, the extent beyond which nothing changed, the global floor, the spill, its half "
                         "radius and decay, written to reach.csv; on the GPU with --device-metrics / --device-alterations (musica_sim_reach); "
                         "without a list, 0 and the half-octaves 1, 2, 3, 4, 6, 8, .. below the image side")
    ap.add_argument("--reach-tables", action="store_true", help="with --reach: keep the exact integers per class in the rows (\"table\")")
    ap.add_argument("--reach-maps", metavar="DIR",
                    help="with --reach: two 8-bit BMPs per row that has a reach into DIR: the class plane and the per-class rmse as bars")
    ap.add_argument("--ensemble", type=int, default=0, metavar="K",
                    help="with --device-alterations: repeat every noise alteration K (1 .. 1024) times and split the change of the output into "
                         "bias against the unaltered result and noise, per pixel, written to ensemble.csv (musica_sim_ensemble_*)")
    ap.add_argument("--ensemble-batch", type=int, default=8, metavar="B", help="with --ensemble: realisations per step of the ensemble context")
    ap.add_argument("--ensemble-maps", metavar="DIR",
                    help="with --ensemble: two 8-bit BMPs per noise row into DIR, one pixel per 64 x 64 tile: the tile's bias rms and its noise rms")
    ap.add_argument("--covariance", type=int, default=0, metavar="R",
                    help="with --ensemble: the spatial auto-covariance of the output noise over the lags within R (1 .. 16) pixels, its "
                         "neighbour correlations, correlation area and noise power spectrum, written to noise_covariance.csv "
                         "(musica_sim_ensemble_track, musica_sim_ensemble_covariance)")
    ap.add_argument("--covariance-maps", metavar="DIR",
                    help="with --covariance: one 8-bit BMP per noise row into DIR: the centred noise power spectrum, log-scaled")
    args = ap.parse_args(argv)
    needs = [(rel.tables, rel.option, "--%s keeps what --%s measures: give --%s" % (rel.tables.replace("_", "-"), rel.option, rel.option)) for rel in RELATIONS]
    needs.insert(5, ("observer", "details", "--observer looks at the details of the cd_ rows: give --details"))   # refused before --point-tables
    for flag, needed, text in needs:
        if getattr(args, flag) and not getattr(args, needed):
            ap.error(text)
    if (args.reach_tables or args.reach_maps) and args.reach is None:
        ap.error("--reach-tables and --reach-maps keep and draw what --reach measures: give --reach")
    if args.covariance and not 1 <= args.covariance <= mp.SIM_MAX_RADIUS:
        ap.error("--covariance takes a radius of 1 .. %d pixels" % mp.SIM_MAX_RADIUS)
    if args.covariance and not args.ensemble:
        ap.error("--covariance is taken over the realisations of an ensemble: give --ensemble")
    if args.covariance_maps and not args.covariance:
        ap.error("--covariance-maps draws what --covariance measures: give a radius")
    if args.ensemble and not 1 <= args.ensemble <= mp.SIM_ENSEMBLE_MAX:
        ap.error("--ensemble takes a count of 1 .. %d realisations" % mp.SIM_ENSEMBLE_MAX)
    if args.ensemble and not args.device_alterations:
        ap.error("--ensemble repeats the device's noise alterations: give --device-alterations")
    if args.ensemble_maps and not args.ensemble:
        ap.error("--ensemble-maps draws what --ensemble measures: give a count")
    if args.ensemble_batch < 1:
        ap.error("--ensemble-batch takes at least 1")
    if args.scales and not 1 <= args.scales <= mp.SIM_MAX_SCALES:
        ap.error("--scales takes a count of 1 .. %d" % mp.SIM_MAX_SCALES)
    if args.displacement and not 1 <= args.displacement <= mp.SIM_MAX_RADIUS:
        ap.error("--displacement takes a radius of 1 .. %d pixels" % mp.SIM_MAX_RADIUS)
    if args.displacement_maps and not args.displacement:
        ap.error("--displacement-maps draws what --displacement measures: give a radius")
    if args.cli and args.device_alterations:
        ap.error("--device-alterations writes the in-process library's input buffer: it cannot be combined with --cli")
    if args.cli and args.device_metrics:
        ap.error("--device-metrics scores the in-process library's device output: it cannot be combined with --cli")
    if args.manifest and (args.raw or args.reference):
        ap.error("--manifest names every raw image and its reference: it cannot be combined with --raw or --reference")
    if args.manifest:
        entries = read_manifest(args.manifest)
    elif args.raw:
        from .processing import read_raw
        raw = read_raw(args.raw, args.size)
        name = os.path.basename(args.raw)
    else:
        from .phantom import phantom
        raw = phantom(args.size, args.phantom_seed, noise=4.0)
        name = "phantom_%d_seed%d" % (args.size, args.phantom_seed)
    if args.reference:
        from .dicom import read_dicom_gray
        vendor = read_dicom_gray(args.reference)
    runner = Runner(args.size, args.levels, use_cli=args.cli, device_metrics=args.device_metrics, device_alterations=args.device_alterations,
                    **({"ensemble_batch": args.ensemble_batch} if args.ensemble else {}))
    shift_args = {"displacement": args.displacement, "displacement_tiles": True} if args.displacement_maps else \
                 {"displacement": args.displacement} if args.displacement else {}
    for m in SCORED_METRICS[1:]:   # --scales .. --minkowski, under their options' names (--tone and --symmetries are passed whatever they say)
        if m.on(getattr(args, m.option)):
            shift_args[m.option] = getattr(args, m.option)
    if args.blobs is not None:
        shift_args["blob_connectivity"] = args.blob_connectivity
    if args.texture is not None:
        shift_args["texture_distances"] = args.texture_distances
    if args.contours is not None:
        shift_args.update(contour_radius=args.contour_radius, contour_maps=bool(args.contour_maps))
    if args.minkowski and args.minkowski_curves:
        shift_args["minkowski_curves"] = True
    for m in MOVED[1:]:                # --blurs .. --codecs: the lists as given, a flag without a list as the entry's defaults for the size
        if getattr(args, m.option):
            shift_args[m.option] = m.cli(getattr(args, m.option), args.size) if m.cli else getattr(args, m.option)
    if args.observer:
        shift_args["observer"] = True
    if args.ensemble:
        shift_args.update(ensemble=args.ensemble, ensemble_tiles=bool(args.ensemble_maps))
    if args.covariance:
        shift_args.update(covariance=args.covariance, covariance_tiles=bool(args.covariance_maps))
    grids = dict(details=DETAILS, edges=EDGES, gratings=GRATINGS, gains=GAINS, points=POINTS)
    for rel in RELATIONS:          # --details .. --points: the defaults for the size, the luts of the image itself (a manifest: of each image)
        if getattr(args, rel.option):
            payloads = (True if args.manifest else LUTS(raw)) if rel.option == "luts" else grids[rel.option](args.size)
            shift_args.update({rel.option: payloads, rel.tables: getattr(args, rel.tables)})
    if args.reach is not None:
        shift_args.update(reach=args.reach, reach_tables=args.reach_tables, reach_maps=bool(args.reach_maps))
    try:
        if args.manifest:
            studies = run_studies(entries, runner, symmetries=args.symmetries, tone=args.tone, **shift_args)
        else:
            studies = [(name, run_study(raw, runner, rng=np.random.default_rng(0), vendor=vendor if args.reference else None,
                                        symmetries=args.symmetries, tone=args.tone, **shift_args))]
    finally:
        runner.close()
    write_studies_csvs(studies, args.out, mean_cnr=not args.cli)
    if args.displacement_maps:
        write_displacement_maps(studies, args.displacement_maps)
    if args.ensemble_maps:
        write_ensemble_maps(studies, args.ensemble_maps)
    if args.covariance_maps:
        write_covariance_maps(studies, args.covariance_maps)
    if args.reach_maps:
        write_reach_maps(studies, args.reach_maps)
    if args.contour_maps and args.contours is not None:
        write_contour_maps(studies, args.contour_maps)
    if args.minkowski_curves and args.minkowski:
        write_minkowski_curves(studies, args.minkowski_curves)
    print("wrote %d alterations to %s" % (sum(len(rows) - 1 for _, rows in studies), args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
