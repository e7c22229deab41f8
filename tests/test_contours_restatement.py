"""The contour metric as the metrics state it (contour_mask, contour_statistics, contour_summary, contour_row), the validators, constants
and prototype that carry it to the library, the host path of a study with `contours` and contour_robustness.csv: everything that needs
no GPU.

contour_statistics is the contract of musica_sim_contours (include/musica.h) and takes its distances from scipy's exact Euclidean
distance transform, by the index of the nearest target pixel; here it is held to a brute-force minimum over all pairs of pixels, to a
pixel-by-pixel restatement of the thinning rule, to every identity that the contract names and to step edges whose answer is known.

Nothing here asserts where a processed image's contours lie: the *_contours values of a row are findings."""
import csv
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

from codec_restatement import StubRunner

TAUS = (1, 4096, 200000)
REACHES = (1, 8, 32)


def step(column, shape=(9, 12), level=100):
    p = np.zeros(shape, dtype=np.uint8)
    p[:, column:] = level
    return p


def mask_literal(p, tau):
    """The thinning rule pixel by pixel, from its definition."""
    h, w = p.shape
    q = p.astype(int)
    M, horizontal = np.zeros((h, w), dtype=int), np.ones((h, w), dtype=bool)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            gx = (q[y - 1, x + 1] + 2 * q[y, x + 1] + q[y + 1, x + 1]) - (q[y - 1, x - 1] + 2 * q[y, x - 1] + q[y + 1, x - 1])
            gy = (q[y + 1, x - 1] + 2 * q[y + 1, x] + q[y + 1, x + 1]) - (q[y - 1, x - 1] + 2 * q[y - 1, x] + q[y - 1, x + 1])
            M[y, x], horizontal[y, x] = gx * gx + gy * gy, abs(gx) >= abs(gy)
    at = lambda x, y: M[y, x] if 0 <= x < w and 0 <= y < h else 0   # noqa: E731
    E = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            before, after = (at(x - 1, y), at(x + 1, y)) if horizontal[y, x] else (at(x, y - 1), at(x, y + 1))
            E[y, x] = M[y, x] >= tau and M[y, x] > before and M[y, x] >= after
    return E, M


def brute_row(S, T, R):
    """All pairs: the minimum squared distance of every pixel of S to the pixels of T."""
    row = np.zeros(R * R + 2, dtype=np.uint64)
    sy, sx = np.nonzero(S)
    ty, tx = np.nonzero(T)
    if len(sy) == 0:
        return row
    if len(ty) == 0:
        row[R * R + 1] = len(sy)
        return row
    d2 = ((sy[:, None] - ty[None, :]) ** 2 + (sx[:, None] - tx[None, :]) ** 2).min(axis=1)
    for v in d2:
        row[v if v <= R * R else R * R + 1] += 1
    return row


def one(a, b, tau, R, region=None, planes=False):
    region = region or (0, 0, 0, 0, a.shape[1], a.shape[0])
    return H.contour_statistics(a, b, [region], tau, R, planes=planes)[0]


# ---- known answers -------------------------------------------------------------------------------------------------------------------------
def test_a_step_edge():
    p = step(6)
    E, M = mask_literal(p, 4096)
    assert (M[1:8, 5] == 160000).all() and (M[1:8, 6] == 160000).all() and M.sum() == 14 * 160000
    assert np.array_equal(H.contour_mask(p, 4096), E)
    assert np.argwhere(E).tolist() == [[y, 5] for y in range(1, 8)]           # column 5 of rows 1 .. 7: seven pixels
    r = one(p, step(9), 4096, 8)
    assert r["contour_a"] == r["contour_b"] == 7 and r["pixels"] == 108 and r["table"].shape == (2, 66) and r["table"].dtype == np.uint64
    assert r["table"][:, 9].tolist() == [7, 7] and r["table"].sum() == 14     # seven pixels at bin 9 in both directions
    r = one(p, step(9), 4096, 2)
    assert r["table"][:, 5].tolist() == [7, 7] and r["table"].sum() == 14     # bin 5 is "far" at R = 2


@pytest.mark.parametrize("shape", [(83, 97), (40, 41), (5, 64)])
def test_the_restatement_against_all_pairs(shape):
    rng = np.random.default_rng(shape[0])
    a, b = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    b[:, shape[1] // 2:] = b[:1, shape[1] // 2:]     # half of b has no horizontal structure: few targets there, long distances
    for tau in TAUS:
        Ea, Eb = mask_literal(a, tau)[0], mask_literal(b, tau)[0]
        assert np.array_equal(H.contour_mask(a, tau), Ea) and np.array_equal(H.contour_mask(b, tau), Eb)
        for R in REACHES:
            r = one(a, b, tau, R, planes=True)
            assert np.array_equal(r["planes"], Ea.astype(np.uint8) | (Eb.astype(np.uint8) << 1)) and r["planes"].dtype == np.uint8
            assert np.array_equal(r["table"], np.stack([brute_row(Ea, Eb, R), brute_row(Eb, Ea, R)])), (tau, R)
            assert r["contour_a"] == int(Ea.sum()) and r["contour_b"] == int(Eb.sum()) and r["pixels"] == shape[0] * shape[1]
            assert "planes" not in one(a, b, tau, R)


# ---- identities ----------------------------------------------------------------------------------------------------------------------------
def test_identities():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (70, 90), dtype=np.uint8)
    b = np.roll(a, (2, 1), axis=(0, 1))
    b[20:30] = rng.integers(0, 256, (10, 90), dtype=np.uint8)
    for tau in TAUS:
        r = one(a, b, tau, 32, planes=True)
        t = r["table"]
        assert t[0].sum() == r["contour_a"] and t[1].sum() == r["contour_b"]
        assert t[0][0] == t[1][0] == int((r["planes"] == 3).sum())
        assert np.array_equal(one(b, a, tau, 32)["table"], t[::-1])                                   # swapping the sides swaps the rows
        same = one(a, a, tau, 32)
        assert same["table"][:, 0].tolist() == [same["contour_a"]] * 2 and not same["table"][:, 1:].any()
        for R in (1, 5, 8, 31):                                                                        # the fold
            folded = np.concatenate([t[:, :R * R + 1], t[:, R * R + 1:].sum(axis=1, keepdims=True)], axis=1)
            assert np.array_equal(one(a, b, tau, R)["table"], folded), (tau, R)
        assert np.array_equal(one(255 - a, b, tau, 32)["table"], t) and np.array_equal(one(a, 255 - b, tau, 32)["table"], t)
        big_a, big_b = np.full((100, 120), 7, np.uint8), np.full((100, 120), 9, np.uint8)              # the same content at another origin
        big_a[11:81, 5:95], big_b[3:73, 17:107] = a, b
        moved = H.contour_statistics(big_a, big_b, [(5, 11, 17, 3, 90, 70)], tau, 32)[0]
        assert np.array_equal(moved["table"], t) and moved["contour_a"] == r["contour_a"]
        sums = set(x * x + y * y for x in range(33) for y in range(33))
        assert not t[:, [i for i in range(32 * 32 + 1) if i not in sums]].any()                        # no sum of two squares: written as 0


# ---- thinning ------------------------------------------------------------------------------------------------------------------------------
def test_thinning_plateau_tie_and_threshold():
    # a plateau: the step between two columns gives two columns of equal strength, the LEFT one is the contour; likewise the UPPER row
    p = step(6)
    assert np.argwhere(H.contour_mask(p, 1)).tolist() == [[y, 5] for y in range(1, 8)]
    assert np.argwhere(H.contour_mask(np.ascontiguousarray(p.T), 1)).tolist() == [[5, x] for x in range(1, 8)]
    # |gx| == |gy|: a diagonal corner is horizontal, so its neighbours along x decide
    q = np.zeros((7, 7), dtype=np.uint8)
    q[np.add.outer(np.arange(7), np.arange(7)) >= 7] = 80
    E, M = mask_literal(q, 1)
    gx, gy = H.sobel_gradients(q)
    assert (np.abs(gx) == np.abs(gy)).all() and np.array_equal(H.contour_mask(q, 1), E) and E.any()
    for y, x in np.argwhere(E):
        assert M[y, x] > M[y, x - 1] and M[y, x] >= M[y, x + 1]
    # M == tau is a contour pixel, M == tau - 1 is not
    assert H.contour_mask(p, 160000).sum() == 7 and H.contour_mask(p, 160001).sum() == 0
    assert H.contour_mask(step(6, level=255), mp.CONTOURS_MAX_THRESHOLD).sum() == 0 and (4 * 255) ** 2 + (2 * 255) ** 2 == mp.CONTOURS_MAX_THRESHOLD


def test_small_regions():
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 256, (12, 12), dtype=np.uint8), rng.integers(0, 256, (12, 12), dtype=np.uint8)
    for w, h in ((1, 1), (2, 2), (1, 8), (9, 2), (2, 3)):       # a side below 3: no contour
        r = one(a, b, 1, 4, (3, 2, 1, 4, w, h), planes=True)
        assert not r["table"].any() and r["contour_a"] == r["contour_b"] == 0 and r["pixels"] == w * h and r["planes"].shape == (h, w)
    r = one(a, b, 1, 4, (3, 2, 1, 4, 3, 3), planes=True)       # 3 x 3: the centre alone has a strength, and it is a maximum
    assert r["contour_a"] == r["contour_b"] == 1 and r["planes"][1, 1] == 3 and r["table"][:, 0].tolist() == [1, 1]
    r = one(a, b, 1, 4, (3, 2, 1, 4, 3, 7))
    assert np.array_equal(r["table"], np.stack([brute_row(*m, 4) for m in ((mask_literal(a[2:9, 3:6], 1)[0], mask_literal(b[4:11, 1:4], 1)[0]),
                                                                           (mask_literal(b[4:11, 1:4], 1)[0], mask_literal(a[2:9, 3:6], 1)[0]))]))
    for bad in ((0, 0, 0, 0, 0, 3), (0, 0, 0, 0, 13, 3), (-1, 0, 0, 0, 3, 3)):
        with pytest.raises(ValueError):
            H.contour_statistics(a, b, [bad], 1, 4)
    with pytest.raises(ValueError):
        H.contour_statistics(a.astype(np.int32), b, [(0, 0, 0, 0, 3, 3)], 1, 4)


# ---- the summary ---------------------------------------------------------------------------------------------------------------------------
def test_summary_on_hand_made_tables():
    R = 3
    t = np.zeros((2, R * R + 2), dtype=np.uint64)
    t[0, [0, 1, 4, 10]] = [4, 2, 1, 3]         # a: ten pixels, three of them far
    t[1, [0, 2, 9]] = [4, 2, 2]                # b: eight pixels, none far
    s = H.contour_summary(t, R, 100)
    assert (s["contour_a"], s["contour_b"], s["density_a"], s["density_b"], s["ratio"]) == (10, 8, 0.1, 0.08, 1.25)
    assert s["fom"] == pytest.approx((4 + 2 / (1 + 1 / 9) + 1 / (1 + 4 / 9)) / 10, rel=1e-15)
    assert (s["kept"], s["moved"], s["lost"], s["spurious"]) == (0.75, 0.25, 0.0, 0.3)
    assert s["a_to_b"] == {"found": 7, "far": 3, "mean": pytest.approx((2 * 1 + 2) / 7), "median": 0.0, "p95": 2.0}
    assert s["b_to_a"] == {"found": 8, "far": 0, "mean": pytest.approx((2 * math.sqrt(2) + 6) / 8), "median": 0.0, "p95": 3.0}
    assert s["hausdorff"] is None              # a has far pixels
    t[0, 10], t[0, 8] = 0, 3
    assert H.contour_summary(t, R, 100)["hausdorff"] == 3.0 and H.contour_summary(t, R, 100)["spurious"] == 0.0
    empty = H.contour_summary(np.zeros((2, 11), dtype=np.uint64), R, 100)
    assert empty["fom"] is None and empty["ratio"] is None and empty["kept"] is None and empty["lost"] is None and empty["spurious"] is None
    assert empty["hausdorff"] is None and empty["a_to_b"] == {"found": 0, "far": 0, "mean": None, "median": None, "p95": None}
    only_a = np.zeros((2, 11), dtype=np.uint64)
    only_a[0, 10] = 5                          # an empty target: everything is far
    s = H.contour_summary(only_a, R, 100)
    assert s["fom"] == 0.0 and s["spurious"] == 1.0 and s["ratio"] is None and s["kept"] is None and s["hausdorff"] is None
    # at R = 1 the diagonal neighbour is not resolved: bin 2 is the far bin and counts as lost, not as kept
    r1 = np.array([[3, 1, 2], [3, 1, 2]], dtype=np.uint64)
    s = H.contour_summary(r1, 1, 50)
    assert (s["kept"], s["moved"], s["lost"]) == (4 / 6, 0.0, 2 / 6)
    same = np.zeros((2, 11), dtype=np.uint64)
    same[:, 0] = 6
    s = H.contour_summary(same, R, 100)
    assert s["fom"] == 1.0 and s["kept"] == 1.0 and s["hausdorff"] == 0.0 and s["a_to_b"]["p95"] == 0.0
    for bad in (np.zeros((2, 10), np.uint64), np.zeros((2, 11)), np.zeros((1, 11), np.uint64)):
        with pytest.raises(ValueError):
            H.contour_summary(bad, R, 100)
    with pytest.raises(ValueError):
        H.contour_summary(same, R, 0)
    row = H.contour_row({"table": t, "pixels": 100}, 4096, R)
    assert list(row)[-4:] == ["threshold", "radius", "pixels", "table"] and row["threshold"] == 4096 and row["radius"] == 3 and row["table"] == t.tolist()
    assert tuple(row)[:len(H.CONTOUR_KEYS) - 1] == H.CONTOUR_KEYS[:-1] and set(H.CONTOUR_KEYS + H.CONTOUR_DIRECTIONS) < set(row)


# ---- the validators, the constants and the prototype -----------------------------------------------------------------------------------------
def test_parameter_helpers_and_their_refusals():
    assert mp.contour_threshold(1) == 1 and mp.contour_threshold(1300500) == 1300500 and mp.contour_threshold(np.int64(4096)) == 4096
    assert mp.contour_radius(1) == 1 and mp.contour_radius(32) == 32 and type(mp.contour_radius(np.uint8(7))) is int
    assert H.mp.contour_threshold is mp.contour_threshold and H.mp.contour_radius is mp.contour_radius
    for bad in (True, False, 4096.0, 1.5, "4096", None, 0, -1, 1300501, (4096,)):
        with pytest.raises(ValueError, match="contours"):
            mp.contour_threshold(bad)
    for bad in (True, 16.0, "16", None, 0, 33, -3, [16]):
        with pytest.raises(ValueError, match="contours"):
            mp.contour_radius(bad)
    assert (mp.CONTOURS_MAX_RADIUS, mp.CONTOURS_MAX_QUERIES, mp.CONTOURS_MAX_THRESHOLD, mp.CONTOURS_THRESHOLD, mp.CONTOURS_RADIUS) == (32, 4, 1300500, 4096, 16)


def test_abi_names_the_call_and_its_struct():
    assert mp.ABI["musica_sim_contours"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(mp.SimQuery), C.POINTER(mp.SimContoursResult),
                                                       C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64])
    assert C.sizeof(mp.SimContoursResult) == 40
    assert [f for f, _ in mp.SimContoursResult._fields_] == ["table_offset", "contour_a", "contour_b", "pixels", "plane_offset"]
    assert hasattr(mp.load_library(), "musica_sim_contours")


def test_the_header_states_the_constants():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "musica.h")).read()
    for name, value in (("MUSICA_CONTOURS_MAX_RADIUS", mp.CONTOURS_MAX_RADIUS), ("MUSICA_CONTOURS_MAX_QUERIES", mp.CONTOURS_MAX_QUERIES)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert re.search(r"#define MUSICA_CONTOURS_MAX_THRESHOLD %du\b" % mp.CONTOURS_MAX_THRESHOLD, text)
    assert "int musica_sim_contours(musica_ctx* ctx, uint32_t threshold, uint32_t radius, uint32_t count, const musica_sim_query* queries," in text
    assert "metrics.contour_statistics" in text


# ---- the study on the host path ----------------------------------------------------------------------------------------------------------
SIDE = 64
STUDY = dict(shutters=[4], translations=[12, 40], rotations=[9], sigmas=[16.0], factors=[0.05], symmetries=(1,))
TAU, REACH = 900, 5


def _study(vendor=None, **kw):
    return H.run_study(phantom(SIDE, 4, noise=4.0), StubRunner(SIDE), rng=np.random.default_rng(2), vendor=vendor, **STUDY, **kw)


@pytest.fixture(scope="module")
def studies():
    vendor = np.random.default_rng(8).integers(0, 65536, size=(SIDE - 20, SIDE - 20), dtype=np.uint16)
    return {(False, None): _study(), (False, TAU): _study(contours=TAU, contour_radius=REACH), (True, None): _study(vendor),
            (True, TAU): _study(vendor, contours=TAU, contour_radius=REACH, granulometry=(1,)), "vendor": vendor}


@pytest.mark.parametrize("with_vendor", [False, True])
def test_run_study_contour_rows(studies, with_vendor):
    plain, scored = studies[(with_vendor, None)], studies[(with_vendor, TAU)]
    assert [r["alteration"] for r in scored] == [r["alteration"] for r in plain]
    siblings = [(c, c + "_contours") for c in H.COMPARED[:4 if with_vendor else 2]]
    for p, t in zip(plain, scored):
        assert not any(k.endswith("_contours") for k in p)
        assert {k: v for k, v in t.items() if not k.endswith(("_contours", "_granulometry"))} == p      # nothing else changes, the noise draws included
    for t in scored:
        mine = [k for k in t if k.endswith("_contours")]
        assert mine == [sib for key, sib in siblings if key in t] == list(t)[-len(mine):]               # behind all other keys, the granulometry's included
        for key, sib in siblings:
            assert (key in t) == (sib in t), (t["alteration"], key)
            if key in t:
                assert (t[sib] is None) == (t[key] is None), (t["alteration"], key)
            if key in t and t[sib] is not None:
                assert tuple(t[sib])[-4:] == ("threshold", "radius", "pixels", "table") and t[sib]["threshold"] == TAU and t[sib]["radius"] == REACH
                assert "planes" not in t[sib]
    by = {r["alteration"]: r for r in scored}
    if with_vendor:
        assert [k for k in by["t_x_12"] if k.endswith("_contours")] == ["direct_contours", "registered_contours", "reference_contours", "registered_reference_contours"]
    unaltered = by["unaltered"]["direct_contours"]
    assert unaltered["pixels"] == 44 * 44 and unaltered["contour_a"] == unaltered["contour_b"] > 0
    assert unaltered["fom"] == 1.0 and unaltered["kept"] == 1.0 and unaltered["hausdorff"] == 0.0 and unaltered["spurious"] == 0.0
    assert by["t_x_40"]["registered"] is None and by["t_x_40"]["registered_contours"] is None and by["t_x_40"]["direct_contours"] is not None
    # the values are contour_statistics of the very images the plain metrics score
    runner = StubRunner(SIDE)
    raw = phantom(SIDE, 4, noise=4.0)
    unalt, alt = runner.run(raw), runner.run(H.clamp_translation(raw, 12, 0))
    side = SIDE - 20
    assert by["t_x_12"]["direct_contours"] == H.contour_row(H.contour_statistics(alt, unalt, [(0, 0, 0, 0, side, side)], TAU, REACH)[0], TAU, REACH)
    region = H.roi_translation_x(unalt.shape, 12)
    assert by["t_x_12"]["registered_contours"] == H.contour_row(H.contour_statistics(alt, unalt, [region], TAU, REACH)[0], TAU, REACH)
    if with_vendor:
        assert by["t_x_12"]["reference_contours"] == H.contour_row(
            H.contour_statistics(alt, H.vendor_to_u8(studies["vendor"]), [(0, 0, 0, 0, side, side)], TAU, REACH)[0], TAU, REACH)


def test_contours_none_is_the_default(studies, tmp_path):
    again = _study(contours=None)
    assert again == studies[(False, None)] and [list(r) for r in again] == [list(r) for r in studies[(False, None)]]
    H.write_studies_csvs([("a.raw", studies[(False, None)])], str(tmp_path / "without"))
    H.write_studies_csvs([("a.raw", again)], str(tmp_path / "none"))
    names = sorted(os.listdir(tmp_path / "without"))
    assert names == sorted(os.listdir(tmp_path / "none")) and "contour_robustness.csv" not in names
    for name in names:
        assert open(tmp_path / "without" / name, "rb").read() == open(tmp_path / "none" / name, "rb").read(), name
    for f in (H.run_study, H.study_options):
        parameters = inspect.signature(f).parameters
        assert parameters["contours"].default is None and parameters["contour_radius"].default == 16 and parameters["contour_maps"].default is False
        assert list(parameters)[-1] == "order"


def test_study_options_contours_and_refusals():
    runner = StubRunner(SIDE)
    args = (SIDE, runner, [], [], [], [], [], None, None, False, 0, False, 0, 0, False, 0, False, None)
    plain = H.study_options(*args)
    assert plain.contours is None and plain.contour_radius == 16 and plain.keys == ("alteration", "direct", "registered", "mean_cnr")
    assert H.study_options(*args, contours=1).keys == ("alteration", "direct", "registered", "mean_cnr", "direct_contours", "registered_contours")
    vendor = np.zeros((SIDE - 20, SIDE - 20), np.uint8)
    opt = H.study_options(SIDE, runner, [], [], [], [], [], vendor, None, True, 3, False, 2, 0, False, 0, False, None, gradients=True, reach=True, order=True, lattice=32,
                          blobs=254, spectrum=64, texture=64, granulometry=[3, 16], contours=np.int32(1300500), contour_radius=32)
    assert opt.contours == 1300500 and type(opt.contours) is int and opt.contour_radius == 32
    assert opt.keys[-5:] == ("registered_reference_granulometry", "direct_contours", "registered_contours", "reference_contours", "registered_reference_contours")
    for bad in (0, 1300501, True, 4096.0, "4096", (4096,)):
        with pytest.raises(ValueError, match="contours"):
            H.study_options(*args, contours=bad)
    for bad in (0, 33, True, 16.0, "16", None):
        with pytest.raises(ValueError, match="contours"):
            H.study_options(*args, contours=4096, contour_radius=bad)
    with pytest.raises(ValueError, match="contour_maps"):
        H.study_options(*args, contours=4096, contour_maps=1)
    # the study walks ROW_METRICS: the earlier tables are its prefix, the new entry is appended behind the granulometry
    assert H.ROW_METRICS[:len(H.STUDY_METRICS)] == H.STUDY_METRICS
    assert [m.option for m in H.ROW_METRICS[len(H.STUDY_METRICS):]] == ["granulometry", "contours"]
    mine = H.ROW_METRICS[-1]
    assert mine.suffix == "contours" and mine.csv is H.METRIC_CSVS["contours"] and mine.csv.file == "contour_robustness.csv"
    assert list(H.METRIC_CSVS)[-1] == "contours"


@pytest.mark.parametrize("with_vendor", [False, True])
def test_contour_csv(studies, tmp_path, with_vendor):
    plain, scored = studies[(with_vendor, None)], studies[(with_vendor, TAU)]
    H.write_studies_csvs([("a.raw", plain)], str(tmp_path / "plain"))
    H.write_studies_csvs([("a.raw", scored), ("b.raw", scored)], str(tmp_path / "scored"))
    assert not os.path.exists(tmp_path / "plain" / "contour_robustness.csv")
    for name in ("direct_robustness.csv", "reg_based_robustness.csv"):
        a = list(csv.reader(open(tmp_path / "plain" / name)))
        b = list(csv.reader(open(tmp_path / "scored" / name)))
        assert a == [r for r in b if r[0] != "b.raw"]                       # the old files do not change
    lines = list(csv.reader(open(tmp_path / "scored" / "contour_robustness.csv")))
    assert lines[0] == H.CONTOUR_CSV_HEADER == ["raw file", "alteration", "comparison", "pixels", "threshold", "radius", "direction", "found", "far", "mean", "median",
                                                "p95", "contour a", "contour b", "density a", "density b", "ratio", "fom", "kept", "moved", "lost", "spurious",
                                                "hausdorff"]
    body = lines[1:]
    keys = [c + "_contours" for c in H.COMPARED]
    want = sum(2 for r in scored for k in keys if r.get(k) is not None)      # a line per comparison and direction
    assert len(body) == 2 * want and all(len(r) == len(lines[0]) for r in body)
    mine = [r for r in body if r[0] == "a.raw" and r[1] == "t_x_12" and r[2] == "registered vs unaltered"]
    t = next(r for r in scored if r["alteration"] == "t_x_12")["registered_contours"]
    assert [r[6] for r in mine] == ["a_to_b", "b_to_a"]
    blank = lambda v: "" if v is None else repr(v)   # noqa: E731
    for r in mine:
        assert r[3:6] == [str(t["pixels"]), str(TAU), str(REACH)]
        assert r[7:12] == [blank(t[r[6]][k]) for k in H.CONTOUR_DIRECTION_KEYS]
        assert r[12:] == [blank(t[k]) for k in H.CONTOUR_KEYS]
    assert not [r for r in body if r[1] == "t_x_40" and r[2] == "registered vs unaltered"]


def test_contour_maps(tmp_path):
    rows = _study(contours=TAU, contour_radius=REACH, contour_maps=True)
    by = {r["alteration"]: r for r in rows}
    planes = by["t_x_12"]["registered_contours"]["planes"]
    region = H.roi_translation_x((SIDE - 20, SIDE - 20), 12)
    assert planes.dtype == np.uint8 and planes.shape == (region[5], region[4]) and planes.max() <= 3
    assert int((planes & 1).sum()) == by["t_x_12"]["registered_contours"]["contour_a"]
    written = H.write_contour_maps([("a.raw", rows)], str(tmp_path))
    assert sorted(os.path.basename(p) for p in written) == sorted("a_%s_contours.bmp" % r["alteration"] for r in rows if r.get("registered_contours") is not None)
    assert os.path.getsize(written[0]) > planes.size // 2


def test_the_command_line_passes_the_options_on(monkeypatch, tmp_path):
    seen = []

    class FakeRunner:
        def __init__(self, *args, **kwargs):
            pass

        def close(self):
            pass

    def fake_study(raw, runner, **kwargs):
        seen.append(tuple(kwargs.get(k, "absent") for k in ("contours", "contour_radius", "contour_maps")))
        return [{"alteration": "unaltered", "direct": None, "registered": None, "mean_cnr": None}]

    monkeypatch.setattr(H, "Runner", FakeRunner)
    monkeypatch.setattr(H, "run_study", fake_study)
    base = ["--size", "64", "--out", str(tmp_path / "out")]
    assert H.main(base + ["--contours"]) == 0 and seen[-1] == (4096, 16, False)
    assert H.main(base + ["--contours", "900", "--contour-radius", "32", "--device-metrics"]) == 0 and seen[-1] == (900, 32, False)
    assert H.main(base + ["--contours", "1300500", "--contour-maps", str(tmp_path / "maps")]) == 0 and seen[-1] == (1300500, 16, True)
    assert H.main(base) == 0 and seen[-1] == ("absent", "absent", "absent")
    assert H.main(base + ["--contour-radius", "3"]) == 0 and seen[-1] == ("absent", "absent", "absent")
    for bad in (["--contours", "0"], ["--contours", "1300501"], ["--contours", "x"], ["--contours", "4096.0"], ["--contours", "--contour-radius", "0"],
                ["--contours", "--contour-radius", "33"], ["--contours", "--contour-radius", "x"]):
        with pytest.raises(SystemExit):
            H.main(base + bad)
