"""The host contract of the edge-response relation (metrics.py: insert_edges, edge_statistics, edge_summary, edge_row; processing.edge_list;
harness.edge_grid and the edge_ rows of run_study), held to independent per-pixel statements in Python integers and fractions, on a CPU.
The device code (kernels_edges.hip) is held to these functions bit for bit in test_gpu_edges.py.

Nothing here asserts how MUSICA renders an edge: the numbers of an edge_ row are findings, not premises."""
import csv
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp

SLOPES = ((1, 4), (3, 4), (1, 16), (15, 16), (5, 13))
CONTRASTS = (512, -512, 1, -1)


def _uv(dx, dy, o):
    return ((dx, dy), (dy, dx), (-dx, dy), (-dy, dx))[o]


def _pixel(v, s, q, c):
    """The contract's pixel in exact rational arithmetic: the absorber covers m / 2q of the aperture, one rounding, halves up."""
    m = min(max(2 * s + q, 0), 2 * q)
    exact = Fraction(v) * (1 - Fraction(c, 1024) * Fraction(m, 2 * q))
    return min(math.floor(exact + Fraction(1, 2)), 65535)


def _insert(image, edges):
    out = [[int(v) for v in row] for row in image]
    for x, y, h, p, q, o, c in edges:
        for py in range(y - 2 * h, y + 2 * h + 1):
            for px in range(x - 2 * h, x + 2 * h + 1):
                u, v = _uv(px - x, py - y, o)
                out[py][px] = _pixel(out[py][px], q * u - p * v, q, c)
    return np.array(out, dtype=np.uint16)


def _u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    return a


def _edges_of_every_kind(n):
    """Four h = 8 plates at pitch 33 from the plane's corner (flush with it) and one h = 9 plate flush with the far corner: with the
    offsets `k` every orientation meets every slope and every contrast over the calls."""
    def lists(k):
        centres = [(16 + 33 * j, 16 + 33 * i) for i in range(2) for j in range(2)]
        es = [(x, y, 8) + SLOPES[(t + k) % 5] + ((t + k // 5) % 4, CONTRASTS[(t + k) % 4]) for t, (x, y) in enumerate(centres)]
        return es + [(n - 19, n - 19, 9) + SLOPES[(4 + k) % 5] + (k % 4, CONTRASTS[k % 4])]
    return [lists(k) for k in range(20)]


def test_insert_edges_is_the_per_pixel_statement():
    n = 104
    image = _u16(n, 1)
    seen = set()
    for edges in _edges_of_every_kind(n)[::3]:
        got = H.insert_edges(image, edges)
        assert got.dtype == np.uint16 and np.array_equal(got, _insert(image, edges))
        assert np.array_equal(H.insert_edges(image, edges[::-1]), got)            # the list's order does not matter
        seen.update((e[3], e[4], e[5]) for e in edges)
    assert {s[:2] for s in seen} == set(SLOPES) and {s[2] for s in seen} == {0, 1, 2, 3}
    assert image[0, 0] == 0 and image[-1, -1] == 65535                            # the input is not written


@pytest.mark.parametrize("v", [0, 1, 2, 65534, 65535])
def test_the_extreme_pixels_under_every_cover(v):
    """v = 0 and 65535 (and their neighbours) at every m of every slope's q, at the extreme contrasts: the u32 bound, the clamp at
    65535 for a void, and the two identities m = 0 -> v, m = 2q -> detail_pixel."""
    image = np.full((33, 33), v, np.uint16)
    for (p, q) in SLOPES:
        for o in range(4):
            for c in CONTRASTS:
                edge = (16, 16, 8, p, q, o, c)
                got = H.insert_edges(image, [edge])
                assert np.array_equal(got, _insert(image, [edge])), edge
                s = H.edge_numerators(8, p, q, o, 16)
                assert s.shape == (33, 33) and (s[16, 16], s[16, 17], s[17, 16]) == tuple(q * a - p * b for a, b in (_uv(0, 0, o), _uv(1, 0, o), _uv(0, 1, o)))
                bare, covered = 2 * s + q <= 0, 2 * s + q >= 2 * q
                assert bare.any() and covered.any() and (~bare & ~covered).any()
                assert (got[bare] == v).all()
                assert (got[covered] == min((v * (1024 - c) + 512) >> 10, 65535)).all()
    assert 65535 * (2048 * 16 + 512 * 32) + 1024 * 16 < 2 ** 32


def _tables(a, b, edge):
    """edge_statistics by a loop over the region's pixels, in Python integers."""
    x, y, h, p, q, o, _ = edge
    big = -((-4 * (q + p) * h) // q)
    t = {k: [0] * (2 * big + 1) for k in mp.EDGE_SUMS}
    ssd = 0
    for py in range(y - h, y + h + 1):
        for px in range(x - h, x + h + 1):
            u, v = _uv(px - x, py - y, o)
            k = (4 * (q * u - p * v)) // q + big
            va, vb = int(a[py, px]), int(b[py, px])
            t["n"][k] += 1
            t["sum_a"][k] += va
            t["sum_b"][k] += vb
            t["sum_aa"][k] += va * va
            ssd += (va - vb) ** 2
    return t, ssd, big


def test_edge_statistics_is_the_brute_force_loop():
    n = 104
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 256, (n, n), dtype=np.uint8), rng.integers(0, 256, (n, n), dtype=np.uint8)
    for edges in _edges_of_every_kind(n)[::4] + [[(51, 52, 25, 5, 13, 3, 7)]]:
        got = H.edge_statistics(a, b, edges)
        assert len(got) == len(edges)
        for s, e in zip(got, edges):
            x, y, h, p, q = e[:5]
            t, ssd, big = _tables(a, b, e)
            assert (s["h"], s["p"], s["q"], s["bins"]) == (h, p, q, 2 * big + 1) and s["bins"] == mp.edge_bins(h, p, q) < 16 * h
            for k in mp.EDGE_SUMS:
                assert s[k].dtype == np.uint32 and s[k].tolist() == t[k], (e, k)
            assert s["roi_ssd"] == ssd and s["roi_pixels"] == (2 * h + 1) ** 2 == int(s["n"].sum())
            assert int(s["sum_a"].sum()) == int(a[y - h:y + h + 1, x - h:x + h + 1].sum())
            assert int(s["n"].max()) <= 2 * h + 1
            c = H.edge_central(h, p, q)
            assert c >= 2 and int(s["n"][big - c:big + c].min()) >= 1               # the central bins are non-empty
            assert type(s["roi_ssd"]) is int and type(s["bins"]) is int


def test_edge_bins():
    assert mp.edge_bins(128, 15, 16) == 1985 and mp.edge_bins(8, 1, 4) == 81 and mp.edge_bins(8, 1, 16) == 2 * 34 + 1
    assert max(mp.edge_bins(128, p, q) for q in range(4, 17) for p in range(1, q)) == 1985 < mp.EDGE_BINS_MAX
    for h, p, q in ((7, 1, 4), (129, 1, 4), (8, 0, 4), (8, 4, 4), (8, 5, 4), (8, 1, 3), (8, 1, 17), (8, 2, 4), (8, 6, 15)):
        assert mp.edge_bins(h, p, q) == 0, (h, p, q)


def test_edge_list_raises_every_refusal():
    n = 200
    ok = ((40, 40, 8, 1, 8, 0, 8), (120, 40, 16, 2, 7, 3, -8))
    assert mp.edge_list(ok, n) == ok and mp.edge_list([list(e) for e in ok], n) == ok
    assert mp.edge_list(((16, 16, 8, 1, 4, 0, 1), (n - 17, n - 17, 8, 1, 4, 0, 1)), n)     # flush with both corners
    bad = {
        "holds 1": [(), [(16 + 33 * (i % 17), 16 + 33 * (i // 17), 8, 1, 4, 0, 1) for i in range(257)]],
        "half-side": [((40, 40, 7, 1, 8, 0, 8),), ((400, 400, 129, 1, 8, 0, 8),)],
        "slope": [((40, 40, 8, 0, 8, 0, 8),), ((40, 40, 8, 8, 8, 0, 8),), ((40, 40, 8, 9, 8, 0, 8),), ((40, 40, 8, 1, 3, 0, 8),),
                  ((40, 40, 8, 1, 17, 0, 8),), ((40, 40, 8, 2, 8, 0, 8),)],
        "orientation": [((40, 40, 8, 1, 8, 4, 8),), ((40, 40, 8, 1, 8, -1, 8),)],
        "contrast": [((40, 40, 8, 1, 8, 0, 0),), ((40, 40, 8, 1, 8, 0, 513),), ((40, 40, 8, 1, 8, 0, -513),)],
        "leaves": [((15, 40, 8, 1, 8, 0, 8),), ((40, 15, 8, 1, 8, 0, 8),), ((n - 16, 40, 8, 1, 8, 0, 8),), ((40, n - 16, 8, 1, 8, 0, 8),), ((-40, 40, 8, 1, 8, 0, 8),)],
        "disjoint": [((40, 40, 8, 1, 8, 0, 8), (72, 40, 8, 1, 8, 0, 8)), ((40, 40, 8, 1, 8, 0, 8), (72, 72, 8, 1, 8, 0, 8)),
                     ((40, 40, 8, 1, 8, 0, 8), (88, 60, 16, 1, 8, 0, 8)), ok + ok[:1]],
        "septuples": [((40, 40, 8, 1, 8, 0),), ((40, 40, 8, 1, 8, 0, 8.5),), 7, ((40, 40, 8, 1, 8, 0, "x"),)],
    }
    for words, lists in bad.items():
        for edges in lists:
            with pytest.raises(ValueError, match=words):
                mp.edge_list(edges, 2000 if words in ("holds 1", "half-side") else n)
    assert mp.edge_list(((40, 40, 8, 1, 8, 0, 8), (73, 40, 8, 1, 8, 0, 8)), n)              # plates that touch are disjoint
    assert mp.edge_list(((40, 40, 8, 1, 8, 0, 0),), n, with_contrast=False)                 # the measurement does not look at c
    image, plane = np.zeros((n, n), np.uint16), np.zeros((n, n), np.uint8)
    for call in (lambda: H.insert_edges(image, ()), lambda: H.insert_edges(plane, ok), lambda: H.insert_edges(image[:, :-1], ok),
                 lambda: H.edge_statistics(plane, plane, ()), lambda: H.edge_statistics(image, image, ok), lambda: H.edge_statistics(plane, plane[:-1, :-1], ok)):
        with pytest.raises(ValueError):
            call()


# ---- edge_summary ----------------------------------------------------------------------------------------------------------------------
def _step_stats(h, p, q, o, low, high, scale=1):
    """The tables of a perfect step: a = low where s < 0, high elsewhere, b = a constant."""
    s = H.edge_numerators(h, p, q, o, 2 * h)                                      # the plane is the edge's plate
    a = (np.where(s < 0, low, high) * scale).astype(np.uint8)
    return H.edge_statistics(a, np.full_like(a, 3 * scale), [(2 * h, 2 * h, h, p, q, o, 0)])


def test_edge_summary_of_a_perfect_step():
    for (h, p, q, o) in ((8, 1, 4, 0), (16, 5, 13, 1), (31, 15, 16, 2), (24, 1, 8, 3)):
        once, twice = H.edge_summary(_step_stats(h, p, q, o, 20, 100))[0], H.edge_summary(_step_stats(h, p, q, o, 20, 100, 2))[0]
        c = H.edge_central(h, p, q)
        assert once["esf"]["k0"] == -c and len(once["esf"]["a"]) == 2 * c and once["esf"]["pitch"] == 0.25 * q / math.sqrt(p * p + q * q)
        assert once["esf"]["a"] == [20.0] * c + [100.0] * c and once["esf"]["b"] == [3.0] * (2 * c) and once["esf"]["d"] == [17.0] * c + [97.0] * c
        for side, step in (("a", 80.0), ("d", 80.0)):
            g = once[side]
            assert set(g) == set(H.EDGE_KEYS)
            assert (g["low"], g["high"], g["step"]) == ((20.0, 100.0, step) if side == "a" else (17.0, 97.0, step))
            assert g["overshoot"] == 0.0 and g["undershoot"] == 0.0
            assert g["rise"] == pytest.approx(0.8 * once["esf"]["pitch"], rel=1e-12)   # one bin, interpolated from 0.1 to 0.9
            assert twice[side]["step"] == 2 * step                                    # doubling a and b doubles the step exactly
            assert twice[side]["overshoot"] == 0.0 and twice[side]["rise"] == g["rise"]
            assert g["mtf_peak"] >= 1.0 and g["mtf50"] is None or g["mtf50"] > 0.4   # an ideal step: flat up to the window's reach
        assert once["b"]["step"] == 0.0 and once["b"]["rise"] is None and once["b"]["overshoot"] is None and once["b"]["mtf50"] is None
        assert once["b"]["mtf_peak"] is None


def test_edge_summary_sees_an_overshoot_and_a_falling_edge():
    esf = [10.0] * 8 + [6.0, 10.0, 50.0, 62.0] + [50.0] * 8                       # undershoot 4 / 40, overshoot 12 / 40
    g = H.edge_profile(esf, 0.25)
    assert (g["low"], g["high"], g["step"]) == (10.0, 50.0, 40.0) and g["undershoot"] == 0.1 and g["overshoot"] == pytest.approx(0.3, rel=1e-12)
    assert g["rise"] == pytest.approx(0.25 * (0.9 - 0.1), rel=1e-12)               # 14 -> 46 lies on the one segment 10 -> 50
    f = H.edge_profile(esf[::-1], 0.25)     # a falling edge: the step is signed; the overshoot is the excursion past the last plateau
    assert f["step"] == -40.0 and f["overshoot"] == pytest.approx(0.1, rel=1e-12) and f["undershoot"] == pytest.approx(0.3, rel=1e-12) and f["rise"] == pytest.approx(g["rise"], rel=1e-12)


def test_mtf_at_zero_is_one():
    rng = np.random.default_rng(4)
    for m in (4, 5, 48, 364, 1984):
        esf = np.cumsum(rng.random(m))
        f, mtf = H.edge_mtf(esf, H.edge_pitch(1, 8))
        assert f[0] == 0.0 and mtf[0] == 1.0 and f[-1] <= 0.5 < f[-1] + f[1] and len(f) == len(mtf)
    assert H.edge_mtf([1.0, 1.0, 1.0, 1.0], 0.25)[1] is None and H.edge_mtf([1.0, 2.0], 0.25)[1] is None


def _gaussian_esf(sigma, h, p, q):
    """The edge-spread function of a step blurred by a Gaussian of sigma pixels, averaged over each bin: the integral of Phi is
    x Phi(x) + sigma^2 phi(x)."""
    pitch, c = H.edge_pitch(p, q), H.edge_central(h, p, q)
    integral = lambda x: x * 0.5 * (1.0 + math.erf(x / (sigma * math.sqrt(2.0)))) + sigma * math.exp(-x * x / (2 * sigma * sigma)) / math.sqrt(2 * math.pi)   # noqa: E731
    return [(integral((k + 1) * pitch) - integral(k * pitch)) / pitch for k in range(-c, c)], pitch


def test_mtf_of_a_gaussian_blurred_step():
    """edge_mtf against the closed form exp(-2 pi^2 sigma^2 f^2) at every frequency up to 0.5 cycles / pixel, sigma = 1 pixel, an
    h = 32 edge of slope 1 / 8 (224 bins of 0.248 pixels). The deviation is the Hann window's: it multiplies the line-spread function,
    so it convolves the MTF with the window's transform. Measured on the CPU: 2.42e-3 (largest, near f = 0.16); the bound is twice
    that, which covers the platform's FFT and erf."""
    esf, pitch = _gaussian_esf(1.0, 32, 1, 8)
    f, mtf = H.edge_mtf(esf, pitch)
    worst = float(np.abs(mtf - np.exp(-2.0 * math.pi ** 2 * f ** 2)).max())
    print("largest deviation of the edge MTF from the closed form: %.3e" % worst)
    assert worst <= 2 * 2.42e-3
    g = H.edge_profile(esf, pitch)
    assert g["mtf50"] == pytest.approx(math.sqrt(math.log(2.0) / 2.0) / math.pi, abs=2e-3)   # exp(-2 pi^2 f^2) = 1/2
    assert g["mtf_peak"] == 1.0 and g["mtf_peak_f"] == 0.0 and g["overshoot"] < 1e-9
    assert g["rise"] == pytest.approx(2 * 1.2815515655, rel=2e-2)                  # the 10-90 % width of a Gaussian edge, 2.563 sigma


# ---- edge_row, edge_grid, the study ----------------------------------------------------------------------------------------------------
def test_edge_row_gathers_and_takes_the_regions_out():
    n = 160
    rng = np.random.default_rng(6)
    a, b = rng.integers(0, 256, (n, n), dtype=np.uint8), rng.integers(0, 256, (n, n), dtype=np.uint8)
    edges = H.output_edges(H.edge_grid(n + 20, 8))
    assert [e[2] for e in edges] == [8, 16, 16, 8] and [e[5] for e in edges] == [0, 1, 2, 3]
    stats = H.edge_statistics(a, b, edges)
    ssd = int(((a.astype(np.int64) - b) ** 2).sum())
    row = H.edge_row(edges, stats, ssd, n * n, tables=True)
    summary = H.edge_summary(stats)
    assert list(row) == ["all", "orientations", "halves", "outside_mse", "per_edge"]
    assert list(row["orientations"]) == [0, 1, 2, 3] and list(row["halves"]) == [8, 16]
    assert row["all"]["edges"] == 4 and row["halves"][16]["edges"] == 2 and row["orientations"][2]["edges"] == 1
    steps = [s["d"]["step"] for s in summary]
    assert row["all"]["step"] == {"min": min(steps), "mean": math.fsum(steps) / 4, "max": max(steps), "count": 4}
    assert row["halves"][16]["step"]["max"] == max(steps[1:3]) and row["orientations"][3]["step"]["mean"] == steps[3]
    inside = sum((2 * e[2] + 1) ** 2 for e in edges)
    assert row["outside_mse"] == (ssd - sum(s["roi_ssd"] for s in stats)) / (n * n - inside)
    assert [(d["x"], d["y"], d["h"], d["p"], d["q"], d["o"], d["c"]) for d in row["per_edge"]] == list(edges)
    assert all(d["esf"] == s["esf"] and d["d"] == s["d"] for d, s in zip(row["per_edge"], summary))
    assert "per_edge" not in H.edge_row(edges, stats, ssd, n * n)
    # a number that no edge of a group has: its spread is empty, not an error
    flat = H.edge_row(edges, H.edge_statistics(a, a, edges), 0, n * n)
    assert flat["all"]["rise"] == {"min": None, "mean": None, "max": None, "count": 0} and flat["all"]["step"]["max"] == 0.0 and flat["outside_mse"] == 0.0


@pytest.mark.parametrize("n, halves, g", [(201, (8, 16), 2), (512, (8, 16, 32), 3), (3072, (8, 16, 32, 64), 8), (53, (8,), 1)])
def test_edge_grid(n, halves, g):
    grids = H.EDGES(n)
    assert [grid[0][6] for grid in grids] == list(H.EDGE_CONTRASTS) == [8, 16, 32, 64, 128]
    grid = grids[0]
    assert len(grid) == g * g and sorted(set(e[2] for e in grid)) == list(halves)
    assert [e[5] for e in grid] == [t % 4 for t in range(g * g)] and [e[3:5] for e in grid] == [H.EDGE_SLOPES[(t // 4) % 4] for t in range(g * g)]
    assert mp.edge_list(grid, n) == grid and mp.edge_list(H.output_edges(grid), n - 20) == H.output_edges(grid)
    for k, h in enumerate(halves):                                                # every half-side equally often in every row of the grid
        assert [sum(1 for e in grid[i * g:(i + 1) * g] if e[2] == h) for i in range(g)] == [g // len(halves)] * g
    assert all(e[:6] == f[:6] for e, f in zip(grids[0], grids[4]))


def test_edge_grid_without_room():
    with pytest.raises(ValueError):
        H.edge_grid(52, 8)
    with pytest.raises(ValueError):
        H.edge_grid(201, 8, halves=(64,))
    assert [e[2] for e in H.edge_grid(201, 8, halves=(9,))] == [9] * 16


SIDE = 160
OUT = SIDE - 2 * H.PROCESSING_MARGIN


class RecordingContext:
    """Stands in for a MusicaProcessing context: logs the name of every sim_* / alter_* / execute* call and answers sim_compare and
    sim_edges from two fixed planes, so the row's "edges" can be recomputed here."""

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

    def _sim_details(self, details, slot, image_index=0):
        return H.detail_statistics(self.a, self.b, details)

    def _alter_edges(self, edges, image_index=0):
        self.lists.append(("alter", tuple(edges)))

    def _sim_edges(self, edges, slot, image_index=0):
        assert slot == H.SLOT_UNALTERED and image_index == 0
        self.lists.append(("sim", tuple(edges)))
        return H.edge_statistics(self.a, self.b, edges)


def _runner(device_alterations):
    r = H.Runner.__new__(H.Runner)
    r.n, r.levels, r.device, r.use_cli = SIDE, 0, 0, False
    r.device_alterations, r.device_metrics, r.ensemble_batch = device_alterations, True, 1
    r.proc, r.ensemble_proc = RecordingContext(), None
    return r


NO_GRIDS = dict(shutters=[], translations=[], rotations=[], sigmas=[], factors=[])


def test_the_edge_rows_of_a_study():
    raw = np.random.default_rng(2).integers(1, 4096, (SIDE, SIDE)).astype(np.uint16)
    grids = H.EDGES(SIDE)[3:]
    details = H.DETAILS(SIDE)[:1]
    runner = _runner(True)
    rows = H.run_study(raw, runner, edges=grids, edge_tables=True, details=details, blurs=[1], **NO_GRIDS)
    log = runner.proc.log
    assert [r["alteration"] for r in rows] == ["unaltered", "blur_1", "cd_8", "edge_64", "edge_128"]   # behind the cd_ rows
    first = log.index("alter_edges")
    assert log[first:] == ["alter_edges", "execute_device", "sim_compare", "sim_edges"] * 2
    assert "alter_edges" not in log[:first] and "sim_edges" not in log[:first]
    assert runner.proc.lists == [("alter", grids[0]), ("sim", H.output_edges(grids[0])), ("alter", grids[1]), ("sim", H.output_edges(grids[1]))]
    p = runner.proc
    ssd = int(((p.a.astype(np.int64) - p.b) ** 2).sum())
    for r, g in zip(rows[3:], grids):
        shifted = H.output_edges(g)
        assert r["edges"] == H.edge_row(shifted, H.edge_statistics(p.a, p.b, shifted), ssd, OUT * OUT, tables=True)
        assert r["registered"] is None and r["direct"] == {k: 0.25 for k in mp.SIM_METRICS} and r["details"] is None
        assert list(r["edges"]["orientations"]) == [0, 1, 2, 3] and len(r["edges"]["per_edge"]) == 4
    assert list(rows[0]) == ["alteration", "direct", "registered", "mean_cnr", "details", "edges"]
    assert all(r["edges"] is None for r in rows[:3])
    # the device-metrics path inserts on the host and measures on the device
    runner = _runner(False)
    rows_m = H.run_study(raw, runner, edges=grids, edge_tables=True, details=details, blurs=[1], **NO_GRIDS)
    log = runner.proc.log
    assert "alter_edges" not in log and log[-3:] == ["execute", "sim_compare", "sim_edges"] and log.count("sim_edges") == 2
    assert [r["edges"] for r in rows_m] == [r["edges"] for r in rows]
    # a study without edges makes no such call and has no such key; its rows are the others' but for the key
    runner = _runner(True)
    plain = H.run_study(raw, runner, details=details, blurs=[1], **NO_GRIDS)
    assert "alter_edges" not in runner.proc.log and "sim_edges" not in runner.proc.log
    assert all("edges" not in r for r in plain)
    assert plain == [{k: v for k, v in r.items() if k != "edges"} for r in rows[:3]]


class HostRunner:
    """Stands in for a Runner on the host path: the "processor" is a fixed function of the raw image (a 3 x 3 box mean of the 8 high
    bits, cropped by the margin), so an inserted edge reaches the output and nothing needs a device."""
    proc, device_metrics, device_alterations = None, False, False

    def run(self, raw):
        v = (np.asarray(raw) >> 4).astype(np.int64)
        box = sum(np.roll(np.roll(v, i, 0), j, 1) for i in (-1, 0, 1) for j in (-1, 0, 1)) // 9
        b = H.PROCESSING_MARGIN
        return np.clip(box[b:-b, b:-b], 0, 255).astype(np.uint8)


def test_the_edge_rows_on_the_host_path():
    raw = (np.random.default_rng(2).integers(0, 64, (SIDE, SIDE)) + 3000).astype(np.uint16)
    grids = H.EDGES(SIDE)
    rows = H.run_study(raw, HostRunner(), rng=np.random.default_rng(1), edges=grids, edge_tables=True, blurs=[1], sigmas=[4.0],
                       shutters=[], translations=[], rotations=[], factors=[])
    plain = H.run_study(raw, HostRunner(), rng=np.random.default_rng(1), blurs=[1], sigmas=[4.0], shutters=[], translations=[], rotations=[], factors=[])
    assert [r["alteration"] for r in rows[len(plain):]] == ["edge_%d" % c for c in H.EDGE_CONTRASTS]
    assert len(rows) == len(plain) + 5 and all("edges" not in r for r in plain)
    assert [{k: v for k, v in r.items() if k != "edges"} for r in rows[:len(plain)]] == plain and all(r["edges"] is None for r in rows[:len(plain)])
    unalt = HostRunner().run(raw)
    for r, g in zip(rows[len(plain):], grids):
        assert list(r) == ["alteration", "direct", "registered", "mean_cnr", "edges"] and r["registered"] is None
        out, shifted = HostRunner().run(H.insert_edges(raw, g)), H.output_edges(g)
        ssd = int(((out.astype(np.int64) - unalt) ** 2).sum())
        assert r["edges"] == H.edge_row(shifted, H.edge_statistics(out, unalt, shifted), ssd, out.size, tables=True)
        assert r["edges"]["outside_mse"] > 0.0                                    # the plates reach h pixels beyond the regions
    # the absorber darkens the s > 0 side of this stand-in's output: a falling edge of about c / 1024 of 187, over about three pixels
    strong = rows[-1]["edges"]["all"]
    assert strong["step"]["count"] == 4 and strong["step"]["max"] < -0.1 * 187 and 1.0 < strong["rise"]["mean"] < 4.0


def test_study_options_refuse_bad_edge_lists_before_any_work():
    raw = np.zeros((SIDE, SIDE), np.uint16)
    runner = _runner(True)
    for grids in ([[(16, 16, 8, 1, 8, 0, 8)]],             # valid for the raw plane, but its plate leaves the output plane
                  [[(60, 60, 8, 1, 8, 0, 0)]], [[(60, 60, 7, 1, 8, 0, 8)]], [[(60, 60, 8, 2, 8, 0, 8)]], [[(60, 60, 8, 1, 8, 4, 8)]],
                  [[(40, 40, 8, 1, 8, 0, 8), (72, 40, 8, 1, 8, 0, 8)]], [[]]):
        with pytest.raises(ValueError):
            H.run_study(raw, runner, edges=grids, **NO_GRIDS)
    assert runner.proc.log == []


def test_edge_response_csv(tmp_path):
    raw = np.random.default_rng(2).integers(1, 4096, (SIDE, SIDE)).astype(np.uint16)
    rows = H.run_study(raw, _runner(True), edges=H.EDGES(SIDE), **NO_GRIDS)
    out = str(tmp_path / "out")
    H.write_studies_csvs([("phantom", rows)], out, mean_cnr=False)
    lines = list(csv.reader(open(os.path.join(out, "edge_response.csv"))))
    assert lines[0] == H.EDGE_CSV_HEADER and len(lines[0]) == 4 + 6 * 4 + 1
    assert [(l[1], l[2], l[3]) for l in lines[1:]] == [("edge_%d" % c, str(o), "1") for c in H.EDGE_CONTRASTS for o in range(4)]
    d = rows[1]["edges"]
    assert lines[1][4:8] == [str(d["orientations"][0]["step"][w]) for w in ("min", "mean", "max", "count")] and lines[1][-1] == str(d["outside_mse"])
    H.write_studies_csvs([("phantom", rows[:1])], str(tmp_path / "plain"), mean_cnr=False)   # an edges study without edge_ rows: the header alone
    assert list(csv.reader(open(os.path.join(str(tmp_path / "plain"), "edge_response.csv")))) == [H.EDGE_CSV_HEADER]
    plain = H.run_study(raw, _runner(True), **NO_GRIDS)
    H.write_studies_csvs([("phantom", plain)], str(tmp_path / "none"), mean_cnr=False)
    assert not os.path.exists(os.path.join(str(tmp_path / "none"), "edge_response.csv"))
