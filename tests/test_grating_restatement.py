"""The host contract of the grating relation (metrics.py: insert_gratings, grating_wave, grating_statistics, grating_summary, grating_row;
processing.grating_list; harness.grating_grid and the grating_ rows of run_study), held to independent per-pixel statements in Python
integers, on a CPU. The device code (kernels_gratings.hip) is held to these functions bit for bit in test_gpu_gratings.py.

Nothing here asserts what gain MUSICA gives a grating: the numbers of a grating_ row are findings, not premises."""
import csv
import math
import os

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp

# (ux, uy, T) for a half-side of 8: both axes with both signs, every quadrant, T = 2, 3, 5
SMALL = ((1, 0, 2), (0, 1, 2), (-1, 0, 3), (0, -1, 5), (1, 1, 2), (1, -1, 3), (-1, 1, 5), (-1, -1, 7), (2, 1, 5), (-1, 2, 5), (-4, -1, 8), (3, -4, 8))
# the eight octants at (8, 3), T = 16
OCTANTS = ((8, 3, 16), (3, 8, 16), (-3, 8, 16), (-8, 3, 16), (-8, -3, 16), (-3, -8, 16), (3, -8, 16), (8, -3, 16))


def _wave(t, seed):
    w = np.random.default_rng(100 * t + seed).integers(-512, 513, t)
    w[0], w[-1] = 512, -512
    if t > 2:
        w[1] = 0
    return tuple(int(v) for v in w)


def _phase(dx, dy, ux, uy, t):
    """The contract's phase: (ux dx + uy dy) mod T, non-negative."""
    k = (ux * dx + uy * dy) % t
    assert 0 <= k < t
    return k


def _insert(image, gratings):
    out = [[int(v) for v in row] for row in image]
    for x, y, h, ux, uy, t, wave in gratings:
        for py in range(y - 2 * h, y + 2 * h + 1):
            for px in range(x - 2 * h, x + 2 * h + 1):
                v = out[py][px]
                # one rounding, halves up: floor(v (1024 - w) / 1024 + 1 / 2), in integers
                out[py][px] = min((2 * v * (1024 - wave[_phase(px - x, py - y, ux, uy, t)]) + 1024) // 2048, 65535)
    return np.array(out, dtype=np.uint16)


def _u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    a[16, 16], a[17, 16], a[16, 17] = 65535, 1, 65535     # under the first plate: saturation, and the smallest non-zero pixel
    return a


def _lists(n):
    """For n >= 84: three h = 8 plates at pitch 33 flush with the plane's corner and one h = 9 plate flush with its far corner, the SMALL
    kinds cycling over the calls; for n >= 137 also an h = 34 plate of every octant."""
    def small(k):
        centres = [(16, 16, 8), (49, 16, 8), (16, 49, 8), (n - 19, n - 19, 9)]
        return [c + SMALL[(i + k) % len(SMALL)][:2] + (SMALL[(i + k) % len(SMALL)][2], _wave(SMALL[(i + k) % len(SMALL)][2], i + k)) for i, c in enumerate(centres)]
    out = [small(k) for k in range(0, len(SMALL), 4)]
    if n >= 137:
        out += [[(68, 68, 34, ux, uy, t, _wave(t, 1))] for ux, uy, t in OCTANTS]
    return out


@pytest.mark.parametrize("n", [84, 137])
def test_insert_gratings_is_the_per_pixel_statement(n):
    image = _u16(n, n)
    saturated = 0
    for gratings in _lists(n):
        got = H.insert_gratings(image, gratings)
        assert got.dtype == np.uint16 and np.array_equal(got, _insert(image, gratings))
        assert np.array_equal(H.insert_gratings(image, gratings[::-1]), got)      # the list's order does not matter
        assert ((got != 0) | (image == 0)).all()                                  # a non-zero pixel stays non-zero
        saturated += int(((got == 65535) & (image < 65535)).sum())
        zero = [g[:6] + ((0,) * g[5],) for g in gratings]
        assert np.array_equal(H.insert_gratings(image, zero), image)              # w = 0 copies
    assert saturated > 0
    assert image[0, 0] == 0 and image[-1, -1] == 65535                            # the input is not written


def test_insert_gratings_at_the_largest_half_side_and_period():
    n = 513
    image = _u16(n, 3)
    for g in ((256, 256, 128, -7, 8, 64, _wave(64, 2)), (256, 256, 128, 0, -1, 2, (512, -512)), (256, 256, 128, 1, 0, 64, _wave(64, 3))):
        assert np.array_equal(H.insert_gratings(image, [g]), _insert(image, [g]))


@pytest.mark.parametrize("v", [0, 1, 2, 3, 65534, 65535])
def test_the_extreme_pixels_under_every_wave_value(v):
    """Against the rounding in floating point-free form: the nearest integer to v (1 - w / 1024), halves up, clipped."""
    image = np.full((33, 33), v, np.uint16)
    for w0 in (-512, -511, -1, 0, 1, 511, 512):
        got = H.insert_gratings(image, [(16, 16, 8, 1, 0, 2, (w0, -w0))])
        for w, px in ((w0, got[16, 16]), (-w0, got[16, 17])):
            want = min((v * (1024 - w) + 512) // 1024, 65535)
            assert px == want and (want > 0 or v == 0), (v, w)
    assert 65535 * 1536 + 512 < 2 ** 32


def _tables(a, b, g):
    x, y, h, ux, uy, t = g[:6]
    d = {"n": [0] * t, "sum_a": [0] * t, "sum_b": [0] * t, "sum_aa": [0] * t}
    ssd = 0
    for py in range(y - h, y + h + 1):
        for px in range(x - h, x + h + 1):
            k, va, vb = _phase(px - x, py - y, ux, uy, t), int(a[py, px]), int(b[py, px])
            d["n"][k] += 1
            d["sum_a"][k] += va
            d["sum_b"][k] += vb
            d["sum_aa"][k] += va * va
            ssd += (va - vb) ** 2
    return d, ssd


@pytest.mark.parametrize("n", [84, 137])
def test_grating_statistics_is_the_brute_force_loop(n):
    rng = np.random.default_rng(n)
    a, b = rng.integers(0, 256, (n, n), dtype=np.uint8), rng.integers(0, 256, (n, n), dtype=np.uint8)
    for gratings in _lists(n):
        stats = H.grating_statistics(a, b, gratings)
        for g, s in zip(gratings, stats):
            want, ssd = _tables(a, b, g)
            assert (s["h"], s["ux"], s["uy"], s["T"]) == g[2:6] and s["roi_ssd"] == ssd and s["roi_pixels"] == (2 * g[2] + 1) ** 2
            for k in mp.GRATING_SUMS:
                assert s[k].dtype == np.uint32 and s[k].tolist() == want[k], (g[:6], k)
        bare = [g[:6] + (None,) for g in gratings]                                # the wave is not looked at
        assert all(np.array_equal(s[k], r[k]) for s, r in zip(stats, H.grating_statistics(a, b, bare)) for k in mp.GRATING_SUMS)


def test_grating_statistics_at_the_largest_half_side_and_period():
    n = 513
    a = np.full((n, n), 255, np.uint8)
    b = np.random.default_rng(1).integers(0, 256, (n, n), dtype=np.uint8)
    for g in ((256, 256, 128, 0, 1, 2, None), (256, 256, 128, -7, 8, 64, None), (256, 256, 128, -1, 0, 64, None)):
        s = H.grating_statistics(a, b, [g])[0]
        want, ssd = _tables(a, b, g)
        assert s["roi_ssd"] == ssd and all(s[k].tolist() == want[k] for k in mp.GRATING_SUMS)
    s = H.grating_statistics(a, b, [(256, 256, 128, 0, 1, 2, None)])[0]
    assert s["n"].tolist() == [129 * 257, 128 * 257] and int(s["sum_aa"][0]) == 33153 * 255 ** 2 > 2 ** 31   # the largest bin there is


def test_every_bin_is_filled_and_bounded_for_every_admissible_grating():
    """The two facts of the contract, exhaustively over (ux, uy, T) at half = max(8, T), the smallest region a period may have:
    every bin is non-empty, and no bin holds more than ceil(S / 2) S pixels, S = 2 half + 1 (so 33153 at most: every sum fits
    uint32)."""
    seen = 0
    fullest = 0.0
    for t in range(2, mp.GRATING_MAX_PERIOD + 1):
        h = max(mp.GRATING_MIN_HALF, t)
        side = 2 * h + 1
        d = np.arange(-h, h + 1)
        for ux in range(-mp.GRATING_MAX_U, mp.GRATING_MAX_U + 1):
            for uy in range(-mp.GRATING_MAX_U, mp.GRATING_MAX_U + 1):
                if not mp.grating_admissible(h, ux, uy, t):
                    continue
                n = np.bincount((np.add.outer(uy * d, ux * d) % t).ravel(), minlength=t)
                assert n.min() > 0 and n.max() <= (side + 1) // 2 * side, (ux, uy, t)
                fullest = max(fullest, n.max() / ((side + 1) // 2 * side))
                seen += 1
    assert seen == 9472 and fullest == 1.0                                        # the bound is attained (T = 2 along an axis)
    assert (2 * mp.GRATING_MAX_HALF + 2) // 2 * (2 * mp.GRATING_MAX_HALF + 1) == 33153 and 33153 * 255 ** 2 < 2 ** 32
    # what admissible means, by hand
    assert mp.grating_admissible(8, 1, 0, 2) and mp.grating_admissible(8, 1, 1, 2) and mp.grating_admissible(128, 8, 7, 64)
    assert not mp.grating_admissible(8, 1, 0, 9) and not mp.grating_admissible(8, 2, 1, 3) and not mp.grating_admissible(8, 0, 0, 4)
    assert not mp.grating_admissible(8, 2, 2, 8) and not mp.grating_admissible(8, 0, 2, 8) and not mp.grating_admissible(128, 1, 0, 65)


def test_grating_list_raises_every_refusal():
    n = 120
    ok = ((40, 40, 8, 1, 0, 8, (0,) * 8), (80, 80, 9, -2, 3, 6, (512, -512, 0, 1, -1, 7)))
    assert mp.grating_list([list(g) for g in ok], n) == ok
    assert mp.grating_list([g[:6] + (None,) for g in ok], n, with_wave=False) == tuple(g[:6] + (None,) for g in ok)
    bad = {
        "septuples": [[(40, 40, 8, 1, 0, 8)], [(40, 40, 8, 1, 0, 8, (0,) * 8, 1)], [(40.5, 40, 8, 1, 0, 8, (0,) * 8)], [(40, 40, 8, 1, 0, 8, (0.5,) * 8)], [(40, 40, 8, 1, 0, 8, None)], [5]],
        "1 .. 256": [[], [(40, 40, 8, 1, 0, 8, (0,) * 8)] * 257],
        "half-side": [[(40, 40, 7, 1, 0, 4, (0,) * 4)], [(300, 300, 129, 1, 0, 8, (0,) * 8)]],
        "wave vector": [[(40, 40, 8, u[0], u[1], 8, (0,) * 8)] for u in ((0, 0), (2, 2), (0, 2), (3, 0), (9, 1), (1, -9), (-4, 2))],
        "period": [[(40, 40, 8, 1, 0, t, (0,) * max(t, 0))] for t in (0, 1, 9, -2)] + [[(300, 300, 128, 1, 0, 65, (0,) * 65)], [(40, 40, 8, 2, 1, 3, (0,) * 3)],
                                                                                       [(40, 40, 8, 1, -3, 5, (0,) * 5)]],
        "the wave": [[(40, 40, 8, 1, 0, 8, (0,) * 7)], [(40, 40, 8, 1, 0, 8, (0,) * 9)], [(40, 40, 8, 1, 0, 8, (513,) + (0,) * 7)], [(40, 40, 8, 1, 0, 8, (0,) * 7 + (-513,))]],
        "leaves": [[(15, 40, 8, 1, 0, 8, (0,) * 8)], [(40, 15, 8, 1, 0, 8, (0,) * 8)], [(n - 16, 40, 8, 1, 0, 8, (0,) * 8)], [(40, n - 16, 8, 1, 0, 8, (0,) * 8)]],
        "disjoint": [[(40, 40, 8, 1, 0, 8, (0,) * 8), (72, 40, 8, 1, 0, 8, (0,) * 8)], [(40, 40, 8, 1, 0, 8, (0,) * 8), (72, 72, 8, 1, 0, 8, (0,) * 8)], list(ok) + [ok[0]]],
    }
    for text, lists in bad.items():
        for gratings in lists:
            with pytest.raises(ValueError, match=text):
                mp.grating_list(gratings, 600 if gratings and gratings[0] != 5 and gratings[0][0] == 300 else n)
    for gratings in bad["the wave"] + [[(40, 40, 8, 1, 0, 8, None)]]:             # the measurement does not look at the wave
        assert len(mp.grating_list(gratings, n, with_wave=False)) == 1
    assert len(mp.grating_list([(16, 16, 8, 1, 0, 8, (0,) * 8), (n - 17, n - 17, 8, 1, 0, 8, (0,) * 8)], n)) == 2   # flush with the plane is inside
    assert len(mp.grating_list([(40, 40, 8, 1, 0, 8, (0,) * 8), (73, 40, 8, 1, 0, 8, (0,) * 8)], n)) == 2           # plates that touch are disjoint
    with pytest.raises(ValueError):
        H.insert_gratings(np.zeros((n, n), np.uint16), [(15, 40, 8, 1, 0, 8, (0,) * 8)])
    with pytest.raises(ValueError):
        H.insert_gratings(np.zeros((n, n), np.uint8), ok)
    with pytest.raises(ValueError):
        H.grating_statistics(np.zeros((n, n), np.uint8), np.zeros((n, n), np.uint16), ok)


def test_grating_wave():
    for t in range(2, mp.GRATING_MAX_PERIOD + 1):
        for c in (1, 7, 8, 16, 32, 64, 127, 128, 511, 512, -8, -511):
            w = H.grating_wave(t, c)
            assert len(w) == t and all(type(v) is int for v in w)
            assert all(w[k] == w[t - k] for k in range(1, t))                     # cos is even about phase 0
            assert w[0] == c and max(abs(v) for v in w) == abs(c)
            if t % 2 == 0:
                assert w[t // 2] == -c
            if t % 4 == 0:
                assert w[t // 4] == 0 == w[3 * t // 4]
            if t % 6 == 0:
                assert w[t // 6] == (c + 1) // 2 and w[t // 3] == (1 - c) // 2    # floor(+-c / 2 + 1 / 2), exactly: ties up for odd c
    assert H.grating_wave(12, 128) == (128, 111, 64, 0, -64, -111, -128, -111, -64, 0, 64, 111)
    assert H.grating_wave(6, 7) == (7, 4, -3, -7, -3, 4) and H.grating_wave(2, -512) == (-512, 512)
    for bad in ((1, 8), (65, 8), (8, 513), (8, -513)):
        with pytest.raises(ValueError):
            H.grating_wave(*bad)


def test_no_wave_entry_hangs_on_the_last_bits_of_a_cosine():
    """Off the substituted points z = c cos(2 pi k / T) is irrational, so z + 1/2 is no integer; over the whole domain it stays at least
    1e-6 away from one, where a libm's cosine is good to about 1e-16 * 512."""
    nearest = 1.0
    for t in range(2, mp.GRATING_MAX_PERIOD + 1):
        for k in range(t):
            if (12 * k) % t == 0 and (12 * k // t) % 2 == 0 or (4 * k) % t == 0:
                continue
            z = np.arange(1, mp.GRATING_MAX_CONTRAST + 1) * math.cos(2.0 * math.pi * k / t) + 0.5
            nearest = min(nearest, float(np.abs(z - np.round(z)).min()))
    assert nearest > 1e-6


def _dft(m):
    """The T Fourier coefficients of one period, O(T^2): X_h = sum_k m_k e^(-2 pi i h k / T)."""
    t = len(m)
    return [complex(math.fsum(v * math.cos(2.0 * math.pi * h * k / t) for k, v in enumerate(m)), -math.fsum(v * math.sin(2.0 * math.pi * h * k / t) for k, v in enumerate(m)))
            for h in range(t)]


def _planes_with_profile(n, g, profile, seed):
    """Two uint8 planes whose difference a - b over the grating's region is profile[k] at every pixel of phase k."""
    x, y, h, ux, uy, t = g[:6]
    b = np.random.default_rng(seed).integers(80, 120, (n, n), dtype=np.uint8)
    a = b.copy()
    k = H.grating_phases(ux, uy, t, h)
    a[y - h:y + h + 1, x - h:x + h + 1] = (b[y - h:y + h + 1, x - h:x + h + 1].astype(np.int64) + np.array(profile)[k]).astype(np.uint8)
    return a, b


REL = 1e-9   # the f64 error of at most 64 terms of magnitude at most 255 is about 1e-12; the margin covers the summation order


def _close(got, want):
    return abs(got - want) <= REL * max(abs(want), 1.0)


@pytest.mark.parametrize("ux, uy, t, h", [(1, 0, 2, 8), (1, 1, 3, 8), (0, 1, 4, 8), (-1, 2, 5, 10), (2, 1, 6, 12), (8, 3, 16, 16), (-7, 8, 64, 64), (1, -1, 33, 40)])
def test_grating_summary_against_an_independent_dft(ux, uy, t, h):
    n = 4 * h + 1
    rng = np.random.default_rng(t)
    profile = [int(v) for v in rng.integers(-60, 61, t)]
    wave = H.grating_wave(t, 64)
    g = (2 * h, 2 * h, h, ux, uy, t, wave)
    a, b = _planes_with_profile(n, g, profile, t)
    stats = H.grating_statistics(a, b, [g])
    s = H.grating_summary(stats, [g])[0]
    assert s["folded"]["d"] == [float(v) for v in profile]                        # exact: n divides sum_a - sum_b
    assert all(_close(m, sa / k) for m, sa, k in zip(s["folded"]["a"], stats[0]["sum_a"].tolist(), stats[0]["n"].tolist()))
    x = _dft(profile)
    assert _close(s["dc"], x[0].real / t)
    for i, hh in enumerate((1, 2, 3)):
        if 2 * hh > t:
            assert s["amplitude"][i] is None and s["harmonic_phase"][i] is None   # the harmonic does not exist
            continue
        want = abs(x[hh]) * (1.0 if 2 * hh == t else 2.0) / t
        assert _close(s["amplitude"][i], want), (hh, s["amplitude"][i], want)
        if want > 1e-6:
            turn = s["harmonic_phase"][i] - math.atan2(x[hh].imag, x[hh].real)
            assert abs(math.remainder(turn, 2.0 * math.pi)) <= 1e-9
    xw = _dft([w / 1024.0 for w in wave])
    win = abs(xw[1]) * (1.0 if t == 2 else 2.0) / t
    assert _close(s["input"], win) and s["response"] == s["amplitude"][0] and _close(s["gain"], s["response"] / win)
    higher = [v for v in s["amplitude"][1:] if v is not None]
    if higher and s["response"] > 0:
        assert _close(s["thd"], math.sqrt(sum(v * v for v in higher)) / s["response"])
    else:
        assert s["thd"] is None
    assert s["roi_mse"] == stats[0]["roi_ssd"] / stats[0]["roi_pixels"]
    sa, sb_, saa, cnt = (stats[0][k].astype(np.int64) for k in ("sum_a", "sum_b", "sum_aa", "n"))
    pooled = sum(int(q) - int(v) ** 2 / int(k) for q, v, k in zip(saa, sa, cnt)) / int(cnt.sum())
    assert _close(s["texture"], pooled) and s["texture"] > 0.0                    # b is random under every phase


def test_grating_summary_of_the_wave_itself():
    """a - b equal to the wave table: the response is 1024 times the input modulation, in phase; to its negative: half a turn away.
    T = 2 is the Nyquist case, one harmonic that takes 1 / T; T = 3: no second harmonic either."""
    for t, u in ((2, (1, 0)), (3, (0, 1)), (4, (1, 1)), (12, (1, -1)), (32, (1, 0))):
        h = H.grating_half(t)
        g = (2 * h, 2 * h, h) + u + (t, H.grating_wave(t, 64))
        for sign, phase in ((1, 0.0), (-1, math.pi)):
            a, b = _planes_with_profile(4 * h + 1, g, [sign * w for w in g[6]], 1)
            s = H.grating_summary(H.grating_statistics(a, b, [g]), [g])[0]
            assert _close(s["gain"], 1024.0) and abs(abs(s["phase"]) - phase) <= 1e-9 and _close(s["dc"], sum(g[6]) * sign / t)
            assert [v is None for v in s["amplitude"]] == [False, t < 4, t < 6]
            assert (s["thd"] is None) == (t < 4) and (s["thd"] is None or s["thd"] < 0.02)   # a rounded cosine has next to no harmonics
    g = (16, 16, 8, 1, 0, 2, (64, -64))
    a, b = _planes_with_profile(33, g, [5, -5], 2)
    s = H.grating_summary(H.grating_statistics(a, b, [g]), [g])[0]
    assert s["amplitude"] == [5.0, None, None] and s["input"] == 0.0625 and s["gain"] == 80.0 and s["dc"] == 0.0
    flat = g[:6] + ((0, 0),)                                                      # no input modulation: no gain, no phase
    s = H.grating_summary(H.grating_statistics(a, b, [flat]), [flat])[0]
    assert s["gain"] is None and s["phase"] is None and s["response"] == 5.0
    s = H.grating_summary(H.grating_statistics(b, b, [g]), [g])[0]                # no response: no distortion figure
    assert s["response"] == 0.0 and s["gain"] == 0.0 and s["thd"] is None and s["roi_mse"] == 0.0


def test_grating_row_gathers_and_takes_the_regions_out():
    n = 140
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 256, (n, n), dtype=np.uint8), rng.integers(0, 256, (n, n), dtype=np.uint8)
    gratings = H.output_gratings(H.grating_grid(n + 20, 32))
    assert len(gratings) == 9
    stats = H.grating_statistics(a, b, gratings)
    ssd = int(((a.astype(np.int64) - b) ** 2).sum())
    row = H.grating_row(gratings, stats, ssd, n * n, tables=True)
    assert list(row) == ["all", "directions", "periods", "outside_mse", "per_grating"]
    assert list(row["directions"]) == ["1,0", "0,1", "1,1", "1,-1"] and list(row["periods"]) == [2, 3, 4]
    assert row["all"]["gratings"] == 9 and sum(g["gratings"] for g in row["periods"].values()) == 9 == sum(g["gratings"] for g in row["directions"].values())
    summary = H.grating_summary(stats, gratings)
    gains = sorted(s["gain"] for s in summary)
    assert row["all"]["gain"] == {"median": gains[4], "min": gains[0], "max": gains[8], "count": 9}
    two = sorted(s["gain"] for g, s in zip(gratings, summary) if (g[3], g[4]) == (1, -1))
    assert len(two) == 2 and row["directions"]["1,-1"]["gain"]["median"] == 0.5 * (two[0] + two[1])
    assert row["periods"][2]["thd"] == {"median": None, "min": None, "max": None, "count": 0}   # T = 2 has no second harmonic
    inside = sum((2 * g[2] + 1) ** 2 for g in gratings)
    mask = np.ones((n, n), bool)
    for g in gratings:
        mask[g[1] - g[2]:g[1] + g[2] + 1, g[0] - g[2]:g[0] + g[2] + 1] = False
    assert mask.sum() == n * n - inside
    assert row["outside_mse"] == int(((a.astype(np.int64) - b)[mask] ** 2).sum()) / int(mask.sum())
    assert [(d["x"], d["y"], d["h"], d["ux"], d["uy"], d["T"], tuple(d["wave"])) for d in row["per_grating"]] == [tuple(g) for g in gratings]
    assert "per_grating" not in H.grating_row(gratings, stats, ssd, n * n)


@pytest.mark.parametrize("n, periods, g", [(201, (2, 3, 4), 3), (512, (2, 3, 4, 6, 8), 5), (3072, H.GRATING_PERIODS, 9), (53, (2,), 1), (160, (2, 3, 4), 3)])
def test_grating_grid(n, periods, g):
    b = H.PROCESSING_MARGIN
    for c in H.GRATING_CONTRASTS:
        grid = H.grating_grid(n, c)
        assert len(grid) == g * g <= mp.GRATING_MAX and sorted(set(x[5] for x in grid)) == list(periods)
        assert all(x[2] == max(8, 2 * x[5]) and x[6] == H.grating_wave(x[5], c) for x in grid)   # at least four periods to a region
        assert all(min(x[0], x[1]) - 2 * x[2] >= b and max(x[0], x[1]) + 2 * x[2] < n - b for x in grid)   # inside the output footprint
        assert [(x[3], x[4]) for x in grid[:4]] == list(H.GRATING_DIRECTIONS)[:len(grid)]   # directions cycle fastest
        cover = np.zeros((n, n), np.int32)
        for x in grid:
            cover[x[1] - 2 * x[2]:x[1] + 2 * x[2] + 1, x[0] - 2 * x[2]:x[0] + 2 * x[2] + 1] += 1
        assert cover.max() == 1                                                   # pairwise disjoint, by counting
        assert mp.grating_list(H.output_gratings(grid), n - 2 * b) == tuple((x[0] - b, x[1] - b) + x[2:] for x in grid)
        counts = {t: sum(1 for x in grid if x[5] == t) for t in periods}
        assert len(set(counts.values())) == 1                                     # every period equally often
    assert H.grating_contrast(H.grating_grid(n, 32)) == 32
    assert [H.grating_contrast(x) for x in H.GRATINGS(n)] == list(H.GRATING_CONTRASTS)


def test_grating_grid_without_room():
    assert H.GRATING_PERIODS == (2, 3, 4, 6, 8, 12, 16, 24, 32) and H.GRATING_DIRECTIONS == ((1, 0), (0, 1), (1, 1), (1, -1))
    assert H.GRATING_CONTRASTS == (8, 16, 32, 64, 128) == H.EDGE_CONTRASTS
    with pytest.raises(ValueError):
        H.grating_grid(52, 8)                                                     # 32 pixels inside the margin: no 33-pixel plate
    with pytest.raises(ValueError):
        H.grating_grid(201, 8, periods=(32,))
    assert len(H.grating_grid(300, 8, periods=(32,))) == 1 and H.grating_grid(300, 8, periods=(32,))[0][2] == 64


# ---- the study -------------------------------------------------------------------------------------------------------------------------
SIDE = 160
OUT = SIDE - 2 * H.PROCESSING_MARGIN


class RecordingContext:
    """Stands in for a MusicaProcessing context: logs the name of every sim_* / alter_* / execute* call and answers sim_compare and
    sim_gratings from two fixed planes, so the row's "gratings" can be recomputed here."""

    def __init__(self):
        rng = np.random.default_rng(9)
        self.a, self.b = rng.integers(0, 256, (OUT, OUT), dtype=np.uint8), rng.integers(0, 256, (OUT, OUT), dtype=np.uint8)
        self.log, self.lists = [], []

    def __getattr__(self, call):
        if not call.startswith(("sim_", "alter_", "execute")):
            raise AttributeError(call)

        def method(*args, **kwargs):
            self.log.append(call)
            return getattr(self, "_" + call, lambda *a, **k: True)(*args, **kwargs)
        return method

    def out_pixels(self, image_index=0):
        return self.a.copy()

    def sync(self):
        pass

    def stats(self, image_index=0):
        class Stats:
            mean_cnr = 0.5
        return Stats

    def _sim_compare(self, queries):
        assert tuple(queries[0]) == (0, H.SLOT_UNALTERED, 0, 0, 0, 0, OUT, OUT)   # the direct comparison comes first
        ssd = int(((self.a.astype(np.int64) - self.b) ** 2).sum())
        return [dict({k: 0.25 for k in mp.SIM_METRICS}, sq_diff_sum=ssd, pixels=OUT * OUT) for _ in queries]

    def _sim_edges(self, edges, slot, image_index=0):
        return H.edge_statistics(self.a, self.b, edges)

    def _alter_gratings(self, gratings, image_index=0):
        self.lists.append(("alter", tuple(gratings)))

    def _sim_gratings(self, gratings, slot, image_index=0):
        assert slot == H.SLOT_UNALTERED and image_index == 0
        self.lists.append(("sim", tuple(gratings)))
        return H.grating_statistics(self.a, self.b, gratings)


def _runner(device_alterations):
    r = H.Runner.__new__(H.Runner)
    r.n, r.levels, r.device, r.use_cli = SIDE, 0, 0, False
    r.device_alterations, r.device_metrics, r.ensemble_batch = device_alterations, True, 1
    r.proc, r.ensemble_proc = RecordingContext(), None
    return r


NO_GRIDS = dict(shutters=[], translations=[], rotations=[], sigmas=[], factors=[])


def test_the_grating_rows_of_a_study():
    raw = np.random.default_rng(2).integers(1, 4096, (SIDE, SIDE)).astype(np.uint16)
    grids = H.GRATINGS(SIDE)[3:]
    edges = H.EDGES(SIDE)[:1]
    runner = _runner(True)
    rows = H.run_study(raw, runner, gratings=grids, grating_tables=True, edges=edges, blurs=[1], **NO_GRIDS)
    log = runner.proc.log
    assert [r["alteration"] for r in rows] == ["unaltered", "blur_1", "edge_8", "grating_64", "grating_128"]   # behind the edge_ rows
    first = log.index("alter_gratings")
    assert log[first:] == ["alter_gratings", "execute_device", "sim_compare", "sim_gratings"] * 2   # one call, behind the row's sim_compare
    assert "alter_gratings" not in log[:first] and "sim_gratings" not in log[:first]
    assert runner.proc.lists == [("alter", grids[0]), ("sim", H.output_gratings(grids[0])), ("alter", grids[1]), ("sim", H.output_gratings(grids[1]))]
    p = runner.proc
    ssd = int(((p.a.astype(np.int64) - p.b) ** 2).sum())
    for r, g in zip(rows[3:], grids):
        shifted = H.output_gratings(g)
        assert r["gratings"] == H.grating_row(shifted, H.grating_statistics(p.a, p.b, shifted), ssd, OUT * OUT, tables=True)
        assert r["registered"] is None and r["direct"] == {k: 0.25 for k in mp.SIM_METRICS} and r["edges"] is None
        assert list(r["gratings"]["periods"]) == [2, 3, 4] and len(r["gratings"]["per_grating"]) == 9
    assert list(rows[0]) == ["alteration", "direct", "registered", "mean_cnr", "edges", "gratings"]
    assert all(r["gratings"] is None for r in rows[:3])
    # the device-metrics path inserts on the host and measures on the device
    runner = _runner(False)
    rows_m = H.run_study(raw, runner, gratings=grids, grating_tables=True, edges=edges, blurs=[1], **NO_GRIDS)
    log = runner.proc.log
    assert "alter_gratings" not in log and log[-3:] == ["execute", "sim_compare", "sim_gratings"] and log.count("sim_gratings") == 2
    assert [r["gratings"] for r in rows_m] == [r["gratings"] for r in rows]
    # a study without gratings makes no such call and has no such key; its rows are the others' but for the key
    runner = _runner(True)
    plain = H.run_study(raw, runner, edges=edges, blurs=[1], **NO_GRIDS)
    assert "alter_gratings" not in runner.proc.log and "sim_gratings" not in runner.proc.log
    assert all("gratings" not in r for r in plain)
    assert plain == [{k: v for k, v in r.items() if k != "gratings"} for r in rows[:3]]
    assert "per_grating" not in H.run_study(raw, _runner(True), gratings=grids[:1], **NO_GRIDS)[1]["gratings"]


class HostRunner:
    """Stands in for a Runner on the host path: the "processor" is a fixed function of the raw image (a 3 x 3 box mean of the 8 high
    bits, cropped by the margin), so an inserted grating reaches the output and nothing needs a device."""
    proc, device_metrics, device_alterations = None, False, False

    def run(self, raw):
        v = (np.asarray(raw) >> 4).astype(np.int64)
        box = sum(np.roll(np.roll(v, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1)) // 9
        b = H.PROCESSING_MARGIN
        return np.clip(box[b:-b, b:-b], 0, 255).astype(np.uint8)


def test_the_grating_rows_on_the_host_path():
    raw = (np.random.default_rng(2).integers(0, 64, (SIDE, SIDE)) + 3000).astype(np.uint16)
    grids = H.GRATINGS(SIDE)
    rows = H.run_study(raw, HostRunner(), rng=np.random.default_rng(1), gratings=grids, grating_tables=True, blurs=[1], sigmas=[4.0],
                       shutters=[], translations=[], rotations=[], factors=[])
    plain = H.run_study(raw, HostRunner(), rng=np.random.default_rng(1), blurs=[1], sigmas=[4.0], shutters=[], translations=[], rotations=[], factors=[])
    assert [r["alteration"] for r in rows[len(plain):]] == ["grating_%d" % c for c in H.GRATING_CONTRASTS]
    assert len(rows) == len(plain) + 5 and all("gratings" not in r for r in plain)
    assert [{k: v for k, v in r.items() if k != "gratings"} for r in rows[:len(plain)]] == plain and all(r["gratings"] is None for r in rows[:len(plain)])
    unalt = HostRunner().run(raw)
    for r, g in zip(rows[len(plain):], grids):
        assert list(r) == ["alteration", "direct", "registered", "mean_cnr", "gratings"] and r["registered"] is None
        out, shifted = HostRunner().run(H.insert_gratings(raw, g)), H.output_gratings(g)
        ssd = int(((out.astype(np.int64) - unalt) ** 2).sum())
        assert r["gratings"] == H.grating_row(shifted, H.grating_statistics(out, unalt, shifted), ssd, out.size, tables=True)
    # this stand-in is linear but for its roundings: a 3 x 3 box passes cos(2 pi x / 4) along an axis at (1 + 2 cos(pi / 2)) / 3 = 1 / 3 of
    # the 189 gray levels under it, darker where the wave attenuates
    strong = [d for d in rows[-1]["gratings"]["per_grating"] if (d["ux"], d["uy"], d["T"]) in ((1, 0, 4), (0, 1, 4))]
    assert strong and all(abs(d["gain"] - 189.0 / 3.0) < 8.0 and abs(abs(d["phase"]) - math.pi) < 0.1 for d in strong)


def test_study_options_refuse_bad_grating_lists_before_any_work():
    raw = np.zeros((SIDE, SIDE), np.uint16)
    runner = _runner(True)
    w = (0,) * 8
    for grids in ([[(16, 16, 8, 1, 0, 8, w)]],             # valid for the raw plane, but its plate leaves the output plane
                  [[(60, 60, 8, 1, 0, 8, (600,) * 8)]], [[(60, 60, 7, 1, 0, 8, w)]], [[(60, 60, 8, 2, 2, 8, w)]], [[(60, 60, 8, 1, 0, 9, (0,) * 9)]],
                  [[(40, 40, 8, 1, 0, 8, w), (72, 40, 8, 1, 0, 8, w)]], [[]]):
        with pytest.raises(ValueError):
            H.run_study(raw, runner, gratings=grids, **NO_GRIDS)
    assert runner.proc.log == []


def test_grating_response_csv(tmp_path):
    raw = np.random.default_rng(2).integers(1, 4096, (SIDE, SIDE)).astype(np.uint16)
    rows = H.run_study(raw, _runner(True), gratings=H.GRATINGS(SIDE), **NO_GRIDS)
    out = str(tmp_path / "out")
    H.write_studies_csvs([("phantom", rows)], out, mean_cnr=False)
    lines = list(csv.reader(open(os.path.join(out, "grating_response.csv"))))
    assert lines[0] == H.GRATING_CSV_HEADER and len(lines[0]) == 4 + 3 * 4 + 1
    assert [(l[1], l[2], l[3]) for l in lines[1:]] == [("grating_%d" % c, str(t), "3") for c in H.GRATING_CONTRASTS for t in (2, 3, 4)]
    d = rows[1]["gratings"]
    assert lines[1][4:8] == [str(d["periods"][2]["gain"][w]) for w in ("median", "min", "max", "count")] and lines[1][-1] == str(d["outside_mse"])
    assert lines[1][8:12] == ["", "", "", "0"]                                    # T = 2 has no distortion figure: empty cells
    H.write_studies_csvs([("phantom", rows[:1])], str(tmp_path / "plain"), mean_cnr=False)   # a gratings study without grating_ rows: the header alone
    assert list(csv.reader(open(os.path.join(str(tmp_path / "plain"), "grating_response.csv")))) == [H.GRATING_CSV_HEADER]
    plain = H.run_study(raw, _runner(True), **NO_GRIDS)
    H.write_studies_csvs([("phantom", plain)], str(tmp_path / "none"), mean_cnr=False)
    assert not os.path.exists(os.path.join(str(tmp_path / "none"), "grating_response.csv"))


def test_the_cli_needs_gratings_for_grating_tables(capsys):
    with pytest.raises(SystemExit):
        H.main(["--grating-tables", "--size", "160"])
    assert "--gratings" in capsys.readouterr().err
