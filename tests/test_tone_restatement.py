"""The joint-histogram tone metrics as harness.py restates them (joint_histogram, tone_lut, tone_similarities: the host side of
musica_sim_joint) against brute-force evaluations of their definitions on small images, their invariance under an invertible remap of
gray levels, the tone=True rows of run_study through a stub runner, and tone_robustness.csv."""
import csv
import math

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

# Summation order only: at most 65536 f64 terms of size <= 1 (entropies: <= ln n / e each) differ by well under 1e-11.
TOL = 1e-9


def _cases():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, size=(48, 64), dtype=np.uint8)
    smooth = (np.add.outer(np.arange(64), np.arange(40)) * 2).astype(np.uint8)
    return {
        "noise_vs_noise": (a, rng.integers(0, 256, size=a.shape, dtype=np.uint8)),
        "correlated": (a, np.clip(a.astype(np.int32) + rng.integers(-9, 10, size=a.shape), 0, 255).astype(np.uint8)),
        "gamma": (smooth, (255.0 * (smooth / 255.0) ** 0.5).astype(np.uint8)),
        "inverted": (smooth, 255 - smooth),
        "few_levels": (rng.integers(7, 11, size=(9, 8), dtype=np.uint8), rng.integers(200, 203, size=(9, 8), dtype=np.uint8)),
        "identical": (a, a.copy()),
        "a_constant": (np.full((16, 20), 77, np.uint8), rng.integers(0, 256, size=(16, 20), dtype=np.uint8)),
        "b_constant": (a, np.full(a.shape, 200, np.uint8)),
        "both_constant": (np.full((8, 8), 3, np.uint8), np.full((8, 8), 250, np.uint8)),
    }


CASES = _cases()


def _brute(a, b):
    """The definitions evaluated directly on the pixels (dictionaries of Python integers, no table)."""
    av, bv = [int(v) for v in a.ravel()], [int(v) for v in b.ravel()]
    n = len(av)
    J, A, B = {}, {}, {}
    for x, y in zip(av, bv):
        J[(x, y)] = J.get((x, y), 0) + 1
        A[x] = A.get(x, 0) + 1
        B[y] = B.get(y, 0) + 1

    def ent(d):
        return -sum(c / n * math.log(c / n) for c in d.values())

    mi = sum(c / n * math.log(c * n / (A[x] * B[y])) for (x, y), c in J.items())
    h_a, h_b = ent(A), ent(B)
    # SSW: the squared distance of every pixel of a to the mean of the a-values that share its b-value; SST: to the mean of a
    ssw = 0.0
    for y in B:
        vals = [x for x, yy in zip(av, bv) if yy == y]
        m = sum(vals) / len(vals)
        ssw += sum((x - m) ** 2 for x in vals)
    mean = sum(av) / n
    sst = sum((x - mean) ** 2 for x in av)
    lut = list(range(256))
    for y in B:
        vals = [x for x, yy in zip(av, bv) if yy == y]
        lut[y] = int(math.floor(sum(vals) / len(vals) + 0.5))     # the means are multiples of 1 / len: exact enough for floor(.. + 0.5)
    return {"mi": mi, "nmi": 1.0 if h_a + h_b == 0 else 2 * mi / (h_a + h_b), "corr_ratio": 1.0 if len(A) == 1 else 1 - ssw / sst,
            "tone_mse": 1 - math.sqrt(ssw / n) / 255, "lut": np.array(lut, dtype=np.uint8), "J": J}


def test_joint_histogram_against_a_double_loop():
    rng = np.random.default_rng(0)
    for shape in [(1, 1), (5, 7), (33, 20)]:
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)
        b = rng.integers(0, 256, size=shape, dtype=np.uint8)
        want = np.zeros((256, 256), dtype=np.int64)
        for i in range(shape[0]):
            for j in range(shape[1]):
                want[a[i, j], b[i, j]] += 1
        got = H.joint_histogram(a, b)
        assert got.shape == (256, 256) and np.array_equal(got, want)
        assert np.array_equal(H.joint_histogram(b, a), want.T)
    with pytest.raises(ValueError):
        H.joint_histogram(np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError):
        H.joint_histogram(np.zeros((4, 4), np.uint16), np.zeros((4, 4), np.uint8))


@pytest.mark.parametrize("name", sorted(CASES))
def test_metrics_against_brute_force(name):
    a, b = CASES[name]
    J = H.joint_histogram(a, b)
    want = _brute(a, b)
    assert {(int(x), int(y)): int(J[x, y]) for x, y in zip(*np.nonzero(J))} == want["J"]
    got = H.tone_similarities(a, b)
    assert tuple(got) == mp.JOINT_METRICS == ("mi", "nmi", "corr_ratio", "tone_mse", "tone_ssim")
    for k in ("mi", "nmi", "corr_ratio", "tone_mse"):
        assert abs(got[k] - want[k]) <= TOL, (name, k, got[k], want[k])
    lut = H.tone_lut(J)
    assert lut.dtype == np.uint8 and lut.shape == (256,)
    # round half up of an exact rational: where the mean is within float noise of k + 1/2 the brute force may round the other way
    B, S, _ = H._joint_moments(J)
    for y in range(256):
        if B[y] and (2 * S[y]) % (2 * B[y]) != B[y]:
            assert lut[y] == want["lut"][y], (name, y)
        elif B[y]:
            assert lut[y] == (S[y] // B[y]) + 1, (name, y)          # exactly half: up
        else:
            assert lut[y] == y
    assert got["tone_ssim"] == H.ssim_similarity(a, lut[b])
    ent = H.joint_similarities(J)
    assert abs(ent["mi"] - (ent["h_a"] + ent["h_b"] - ent["h_ab"])) <= TOL          # I(a; b) = H(a) + H(b) - H(a, b)


def test_special_cases():
    a, b = CASES["identical"]
    r = H.tone_similarities(a, b)
    assert r["corr_ratio"] == 1.0 and r["tone_mse"] == 1.0 and abs(r["nmi"] - 1.0) <= TOL
    assert np.array_equal(H.tone_lut(H.joint_histogram(a, b))[b], a) and abs(r["tone_ssim"] - 1.0) <= 1e-12
    a, b = CASES["a_constant"]
    r = H.tone_similarities(a, b)
    assert r["mi"] == 0.0 and r["corr_ratio"] == 1.0 and r["tone_mse"] == 1.0      # nothing to explain: SST's numerator is 0
    assert np.array_equal(H.tone_lut(H.joint_histogram(a, b))[b], a)
    a, b = CASES["b_constant"]
    r = H.tone_similarities(a, b)
    assert abs(r["mi"]) <= TOL and abs(r["nmi"]) <= TOL and abs(r["corr_ratio"]) <= TOL
    assert abs(r["tone_mse"] - (1.0 - float(np.std(a.astype(np.float64))) / 255.0)) <= TOL
    a, b = CASES["both_constant"]
    r = H.tone_similarities(a, b)
    assert r["mi"] == 0.0 and r["nmi"] == 1.0 and r["corr_ratio"] == 1.0 and r["tone_mse"] == 1.0
    # independent uniform noise: mi is the estimator's bias, about (256 - 1)^2 / (2 n) nats, far below the 5.5 nats of a == b
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, size=(1024, 1024), dtype=np.uint8)
    b = rng.integers(0, 256, size=(1024, 1024), dtype=np.uint8)
    r = H.tone_similarities(a[:256, :256], b[:256, :256])
    big = H.joint_similarities(H.joint_histogram(a, b))
    assert 0.0 <= big["mi"] < 0.05 and big["nmi"] < 0.01 and abs(big["corr_ratio"]) < 0.001
    assert big["mi"] < r["mi"] < 1.0                                                # the bias falls with n
    # an inverted image is a function of the original: everything the remap can explain, it explains
    a, b = CASES["inverted"]
    r = H.tone_similarities(a, b)
    assert r["corr_ratio"] == 1.0 and r["tone_mse"] == 1.0 and abs(r["nmi"] - 1.0) <= TOL and H.mse_similarity(a, b) < 0.7


@pytest.mark.parametrize("name", ["noise_vs_noise", "correlated", "gamma", "few_levels", "b_constant"])
def test_invariance_under_a_permutation_of_gray_levels(name):
    a, b = CASES[name]
    perm = np.random.default_rng(17).permutation(256).astype(np.uint8)
    J, Jp = H.joint_histogram(a, b), H.joint_histogram(a, perm[b])
    want = np.zeros_like(J)
    want[:, perm] = J                       # column b of J is column perm[b] of the permuted table
    assert np.array_equal(Jp, want)
    r, rp = H.joint_similarities(J), H.joint_similarities(Jp)
    for k in ("mi", "nmi", "corr_ratio", "tone_mse"):
        assert abs(r[k] - rp[k]) <= TOL, (name, k, r[k], rp[k])
    assert np.array_equal(H.tone_lut(Jp)[perm[b]], H.tone_lut(J)[b])     # the tone-matched image is the same image


@pytest.mark.parametrize("name", sorted(CASES))
def test_tone_mse_is_at_least_mse(name):
    """The identity is one of the remaps, so the best remap leaves no more squared error than none: as exact integers,
    SSW's numerators summed over a common denominator <= the sum of squared differences."""
    from fractions import Fraction
    a, b = CASES[name]
    J = H.joint_histogram(a, b)
    B, S, Q = H._joint_moments(J)
    ssd = int(np.sum((a.astype(np.int64) - b.astype(np.int64)) ** 2))
    d = np.arange(256)
    assert int(np.sum(J * np.subtract.outer(d, d) ** 2)) == ssd
    ssw = sum(Fraction(B[y] * Q[y] - S[y] * S[y], B[y]) for y in range(256) if B[y])
    assert 0 <= ssw <= ssd
    assert all(B[y] * Q[y] >= S[y] * S[y] for y in range(256))
    assert H.tone_similarities(a, b)["tone_mse"] >= H.mse_similarity(a, b) - 1e-12


class StubRunner:
    """harness.Runner's interface with a stand-in for the pipeline whose tone curve follows the image's own histogram, as MUSICA's
    gradation does: the cropped image, histogram-equalised to 8 bits."""

    def __init__(self, n):
        self.n = n
        self.proc = self
        self._last = None

    def run(self, raw, workdir=None):
        m = H.PROCESSING_MARGIN
        crop = raw[m:-m, m:-m]
        ranks = np.searchsorted(np.sort(crop.ravel()), crop.ravel(), side="right").reshape(crop.shape)
        self._last = (255.0 * (ranks - 1) / max(crop.size - 1, 1)).astype(np.uint8)
        return self._last

    def mean_cnr(self):
        return float(self._last.mean())


def _stub_study(tone, vendor=None, **kw):
    n = 128
    raw = phantom(n, 4, noise=4.0)
    args = dict(shutters=[10], translations=[12, 125], rotations=[9], sigmas=[16.0], factors=[0.05], symmetries=(1, 4))
    args.update(kw)
    rows = H.run_study(raw, StubRunner(n), rng=np.random.default_rng(2), vendor=vendor, **({"tone": True} if tone else {}), **args)
    return raw, rows


def _same(x, y):
    if isinstance(x, dict):
        return isinstance(y, dict) and list(x) == list(y) and all(_same(x[k], y[k]) for k in x)
    return x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y))


@pytest.mark.parametrize("with_vendor", [False, True])
def test_run_study_tone_rows(with_vendor):
    n = 128
    vendor = np.random.default_rng(8).integers(0, 65536, size=(n - 20, n - 20), dtype=np.uint16) if with_vendor else None
    raw, plain = _stub_study(False, vendor)
    _, toned = _stub_study(True, vendor)
    assert [r["alteration"] for r in toned] == [r["alteration"] for r in plain]
    pairs = [("direct", "direct_tone"), ("registered", "registered_tone")] + \
            ([("reference", "reference_tone"), ("registered_reference", "registered_reference_tone")] if with_vendor else [])
    assert H.TONE_KEYS == {"direct": "direct_tone", "registered": "registered_tone", "reference": "reference_tone",
                           "registered_reference": "registered_reference_tone"} and H.SLOT_TONE == 4
    some_registered = some_unregistered = False
    for p, t in zip(plain, toned):
        # tone=False rows are today's: no new key; tone=True adds the siblings and changes nothing else
        assert not any(k.endswith("_tone") for k in p)
        assert _same({k: v for k, v in t.items() if not k.endswith("_tone")}, p)
        for key, sib in pairs:
            assert (key in t) == (sib in t), (t["alteration"], key)
            if key not in t:
                continue
            assert (t[key] is None) == (t[sib] is None), (t["alteration"], key)
            if t[sib] is not None:
                assert tuple(t[sib]) == mp.JOINT_METRICS and all(isinstance(v, float) for v in t[sib].values())
        assert not any(k.endswith("_tone") and k not in H.TONE_KEYS.values() for k in t)
        some_registered |= t["registered_tone"] is not None
        some_unregistered |= t["alteration"] != "unaltered" and t["registered_tone"] is None
    assert some_registered and some_unregistered          # t_x_125 leaves a 3-pixel strip: no registration
    by = {r["alteration"]: r for r in toned}
    assert "registered_reference" not in by["unaltered"] and "registered_reference_tone" not in by["unaltered"]
    assert by["unaltered"]["direct_tone"]["corr_ratio"] == 1.0 and by["unaltered"]["direct_tone"]["tone_mse"] == 1.0
    # the values are tone_similarities of the very images the plain metrics score
    runner = StubRunner(n)
    unalt = runner.run(raw)
    alt = runner.run(H.clamp_translation(raw, 12, 0))
    assert by["t_x_12"]["direct_tone"] == H.tone_similarities(alt, unalt)
    assert by["t_x_12"]["registered_tone"] == H.tone_similarities(*H.register_translation_x(alt, unalt, 12))
    if with_vendor:
        assert by["t_x_12"]["reference_tone"] == H.tone_similarities(alt, H.vendor_to_u8(vendor))
    # the histogram-driven stand-in moves its tone curve under a shutter: removing tone recovers what mse charged for it
    c = by["c_sh_10"]
    assert c["registered_tone"]["tone_mse"] >= c["registered"]["mse"]


def test_tone_false_is_the_default_and_draws_the_same_noise():
    _, a = _stub_study(False)
    n = 128
    rows = H.run_study(phantom(n, 4, noise=4.0), StubRunner(n), rng=np.random.default_rng(2), shutters=[10], translations=[12, 125],
                       rotations=[9], sigmas=[16.0], factors=[0.05], symmetries=(1, 4), tone=False)
    assert all(_same(x, y) for x, y in zip(a, rows)) and len(a) == len(rows)


@pytest.mark.parametrize("with_vendor", [False, True])
def test_tone_csv(tmp_path, with_vendor):
    n = 128
    vendor = np.random.default_rng(8).integers(0, 256, size=(n - 20, n - 20), dtype=np.uint8) if with_vendor else None
    _, plain = _stub_study(False, vendor)
    _, toned = _stub_study(True, vendor)
    H.write_studies_csvs([("a.raw", plain)], str(tmp_path / "plain"))
    H.write_studies_csvs([("a.raw", toned), ("b.raw", toned)], str(tmp_path / "toned"))
    assert not (tmp_path / "plain" / "tone_robustness.csv").exists()
    H.write_study_csvs(toned, str(tmp_path / "one"), "a.raw")
    for name in ("direct_robustness.csv", "reg_based_robustness.csv", "mean_cnr.csv") + (("ref_similarities.csv",) if with_vendor else ()):
        assert (tmp_path / "one" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name   # the other files keep their bytes
    t = list(csv.reader(open(tmp_path / "toned" / "tone_robustness.csv")))
    groups = 4 if with_vendor else 2
    assert t[0] == H.tone_csv_header(with_vendor) and len(t[0]) == 2 + 5 * groups and t[0][:2] == ["raw file", "alteration"]
    assert len(set(t[0])) == len(t[0])
    assert len(t) == 1 + 2 * len(toned)
    assert [r[0] for r in t[1:]] == ["a.raw"] * len(toned) + ["b.raw"] * len(toned)
    keys = ["direct_tone", "registered_tone", "reference_tone", "registered_reference_tone"][:groups]
    for line, row in zip(t[1:], toned):
        assert line[1] == row["alteration"] and len(line) == len(t[0])
        for g, key in enumerate(keys):
            cells = line[2 + 5 * g:7 + 5 * g]
            if row.get(key) is None:
                assert cells == [""] * 5
            else:
                assert [float(c) for c in cells] == [row[key][k] for k in mp.JOINT_METRICS]
