"""Scale-resolved SSIM on the device (musica_sim_multiscale; kernels_scales.hip) against harness.multiscale_similarities: the exact
quantities (ssd per scale, plane sizes) bit for bit, the f64 ones to round-off, scale 0 against musica_sim_compare, the extremes, the
Kronecker property, the refusals, what the call leaves untouched, and device studies with scales=5 against the host-scored one.

Everything runs at n = 532 (512 x 512 outputs). The full frame is wider than one 64-pixel pooling tile at every scale and than one
250-column strip of the windowed launch at scales 0 and 1 (a strip of scale 4 would take a region 4000 pixels wide)."""
import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom
from test_gpu_similarity import _graded_plane

pytestmark = pytest.mark.gpu

TOL = 1e-12
N = 532
NW = N - 2 * mp.OUT_MARGIN
BATCH = 3

# (image_index, slot, ax, ay, bx, by, w, h), every one at 5 scales in one call
QUERIES5 = [(0, 0, 0, 0, 0, 0, NW, NW),                  # the full frame: 8 x 32 tiles, 3 strips at scale 0, 2 at scale 1
            (1, 1, 0, 0, 0, 0, NW, NW),                  # correlated planes: SSIM near 1
            (2, 5, 3, 7, 9, 1, 500, 301),                # ragged, odd and unequal offsets
            (1, 1, 13, 250, 257, 7, 255, 129),           # 129 >> 4 == 8
            (2, 0, 301, 5, 0, 399, 112, 112),            # a single window at scale 4
            (1, 5, 17, 33, 2, 91, 113, 127),             # dropped rows and columns differ per scale
            (0, 1, 1, 399, 399, 1, 113, 112)]
QUERIES1 = [(0, 5, NW - 7, NW - 7, 0, 0, 7, 7), (1, 1, 505, 3, 3, 505, 7, 7), (2, 1, 1, 2, 3, 4, 255, 9), (2, 0, 0, 0, 0, 0, NW, NW)]
QUERIES3 = [(2, 1, 1, 2, 3, 4, 255, 29), (0, 0, 100, 101, 7, 0, 28, 300)]      # 29 >> 2 == 7: one row of windows at the last scale


def _ctx(batch=BATCH):
    p = mp.MusicaProcessing()
    assert p.init(N, levels=0, batch=batch, flags=mp.FLAG_NO_AUTOTUNE), mp.last_error()
    return p


def _crop(img, x, y, w, h):
    return img[y:y + h, x:x + w]


@pytest.fixture(scope="module")
def scene():
    """One context with injected graded planes and three slots; the device results of the three calls and the host's, computed once."""
    rng = np.random.default_rng(17)
    p = _ctx()
    for i in range(BATCH):
        p.set_image(mp.IMG_GRADED, 0, _graded_plane(N, rng), image_index=i)
    outs = [p.out_pixels(i) for i in range(BATCH)]
    slots = {0: rng.integers(0, 256, size=(NW, NW), dtype=np.uint8),
             1: np.clip(outs[1].astype(np.int32) + rng.integers(-6, 7, size=(NW, NW)), 0, 255).astype(np.uint8),
             5: rng.integers(40, 90, size=(NW, NW), dtype=np.uint8)}
    for s, v in slots.items():
        p.sim_set_reference(s, v)
    calls = {5: QUERIES5, 1: QUERIES1, 3: QUERIES3}
    dev = {n: p.sim_multiscale(qs, n) for n, qs in calls.items()}
    host = {n: [H.multiscale_similarities(_crop(outs[q[0]], q[2], q[3], q[6], q[7]), _crop(slots[q[1]], q[4], q[5], q[6], q[7]), n) for q in qs]
            for n, qs in calls.items()}
    yield {"p": p, "outs": outs, "slots": slots, "calls": calls, "dev": dev, "host": host}
    p.cleanup()


def _check(r, want, what):
    n = want["scales"]
    assert r["scales"] == n and r["pixels"] == want["pixels"], what
    for k in ("ssd", "plane_w", "plane_h"):
        assert r[k] == want[k], (what, k, r[k], want[k])                      # bit for bit
        assert r["raw"][k][n:] == [0] * (mp.SIM_MAX_SCALES - n), (what, k)   # entries at s >= scales are zero
    for k in mp.SCALE_METRICS:
        print(what, k, [abs(a - b) for a, b in zip(r[k], want[k])])
        assert len(r[k]) == n and all(abs(a - b) <= TOL for a, b in zip(r[k], want[k])), (what, k, r[k], want[k])
        assert r["raw"][k][n:] == [0.0] * (mp.SIM_MAX_SCALES - n), (what, k)
    assert abs(r["ms_ssim"] - want["ms_ssim"]) <= TOL, (what, r["ms_ssim"], want["ms_ssim"])


@pytest.mark.parametrize("scales", [5, 1, 3])
def test_matches_the_restatement(scene, scales):
    for q, r, want in zip(scene["calls"][scales], scene["dev"][scales], scene["host"][scales]):
        _check(r, want, str(q))


def test_scale_0_is_musica_sim_compare(scene):
    for n, qs in scene["calls"].items():
        for q, r, c in zip(qs, scene["dev"][n], scene["p"].sim_compare(qs)):
            assert r["ssd"][0] == c["sq_diff_sum"] and r["pixels"] == c["pixels"], q
            assert abs(r["ssim"][0] - c["ssim"]) <= TOL and abs(r["mse"][0] - c["mse"]) <= TOL, (q, r["ssim"][0], c["ssim"])


def test_a_second_call_is_bit_identical_and_nothing_else_changed(scene):
    p = scene["p"]
    for n, qs in scene["calls"].items():
        assert p.sim_multiscale(qs, n) == scene["dev"][n]
    # a call of one query gives that query's numbers: a result does not depend on its neighbours in the call
    assert p.sim_multiscale([QUERIES5[2]], 5)[0] == scene["dev"][5][2]
    for s, v in scene["slots"].items():
        assert np.array_equal(p.sim_get_reference(s), v)
    for i in range(BATCH):
        assert np.array_equal(p.out_pixels(i), scene["outs"][i])


def test_extremes():
    p = _ctx(batch=2)
    assert p.execute(np.stack([phantom(N, 3, noise=4.0), phantom(N, 4, noise=4.0)])), mp.last_error()
    for i in range(2):
        p.sim_capture(3, i)                       # a captured output against itself: exactly 1 at every scale
        r = p.sim_multiscale([(i, 3, 0, 0, 0, 0, NW, NW), (i, 3, 5, 9, 5, 9, 301, 500)], 5)
        for one in r:
            assert one["ssim"] == [1.0] * 5 and one["cs"] == [1.0] * 5 and one["lum"] == [1.0] * 5 and one["mse"] == [1.0] * 5
            assert one["ssd"] == [0] * 5 and one["ms_ssim"] == 1.0
    # all-255 against alternating 0 / 255 rows, 112 x 112: the window sums reach their u64 maxima at scale 4
    p.set_image(mp.IMG_GRADED, 0, np.ones((N, N), dtype=np.float32), image_index=1)
    a = p.out_pixels(1)
    assert np.all(a == 255)
    b = np.full((NW, NW), 255, dtype=np.uint8)
    b[::2] = 0
    p.sim_set_reference(0, b)
    for q in ((1, 0, 0, 0, 0, 0, 112, 112), (1, 0, 7, 3, 5, 10, 112, 112), (1, 0, 0, 0, 0, 0, NW, NW)):
        r = p.sim_multiscale([q], 5)[0]
        want = H.multiscale_similarities(_crop(a, q[2], q[3], q[6], q[7]), _crop(b, q[4], q[5], q[6], q[7]), 5)
        _check(r, want, str(q))
        assert r["ssd"][4] == (q[6] >> 4) * (q[7] >> 4) * (255 * 128) ** 2 and r["cs"][1:] == [1.0] * 4 and r["mse"][1:] == [0.5] * 4
    same = p.sim_multiscale([(1, 0, 0, 0, 0, 0, 112, 112)], 5)[0]       # the slot itself is not all-255: set one that is
    p.sim_set_reference(1, np.full((NW, NW), 255, dtype=np.uint8))
    r = p.sim_multiscale([(1, 1, 0, 0, 400, 400, 112, 112)], 5)[0]
    assert r["ssim"] == [1.0] * 5 and r["cs"] == [1.0] * 5 and r["lum"] == [1.0] * 5 and r["ms_ssim"] == 1.0 and same["ms_ssim"] < 1.0
    p.cleanup()


def test_kronecker_property():
    """A slot and an injected plane built with np.kron(., ones((16, 16))): scale 4 of the pair is scale 0 of the small pair."""
    rng = np.random.default_rng(23)
    small = NW // 16
    A = rng.integers(0, 256, size=(small, small), dtype=np.uint8)
    B = np.clip(A.astype(np.int32) + rng.integers(-40, 41, size=A.shape), 0, 255).astype(np.uint8)
    ones = np.ones((16, 16), dtype=np.uint8)
    p = _ctx(batch=2)

    def inject(index, values):
        """`values` (NW x NW u8) as image `index`'s output."""
        full = np.zeros((N, N), dtype=np.float64)
        full[mp.OUT_MARGIN:-mp.OUT_MARGIN, mp.OUT_MARGIN:-mp.OUT_MARGIN] = values
        p.set_image(mp.IMG_GRADED, 0, ((full + 0.5) / 255.0).astype(np.float32), image_index=index)
        assert np.array_equal(p.out_pixels(index), values)

    corner_a, corner_b = np.zeros((NW, NW), dtype=np.uint8), np.zeros((NW, NW), dtype=np.uint8)
    corner_a[:small, :small], corner_b[:small, :small] = A, B
    inject(0, np.kron(A, ones))
    inject(1, corner_a)
    p.sim_set_reference(0, np.kron(B, ones))
    p.sim_set_reference(1, corner_b)
    big = p.sim_multiscale([(0, 0, 0, 0, 0, 0, NW, NW)], 5)[0]
    ref = p.sim_compare([(1, 1, 0, 0, 0, 0, small, small)])[0]
    one = p.sim_multiscale([(1, 1, 0, 0, 0, 0, small, small)], 1)[0]
    assert abs(big["ssim"][4] - ref["ssim"]) <= TOL
    _check(big, H.multiscale_similarities(np.kron(A, ones), np.kron(B, ones), 5), "kron")
    assert abs(big["ssim"][4] - one["ssim"][0]) <= TOL and abs(big["cs"][4] - one["cs"][0]) <= TOL and abs(big["lum"][4] - one["lum"][0]) <= TOL
    assert big["ssd"][4] == 65536 * one["ssd"][0] and abs(big["mse"][4] - one["mse"][0]) <= TOL
    p.cleanup()


GOOD = (0, 0, 0, 0, 0, 0, 200, 200)
REFUSALS = [("ctx", "NULL"), ("queries", "NULL"), ("results", "NULL"), ("count0", "count"), ("count65", "count"), ("scales0", "scales"),
            ("scales6", "scales"), ((0, 0, 0, 0, 0, 0, 111, 200), "7 x 7"), ((0, 0, 0, 0, 0, 0, 200, 111), "7 x 7"),
            ((0, 0, 0, 0, 0, 0, 6, 200), "7 x 7"), ((0, 8, 0, 0, 0, 0, 200, 200), "slot"), ((0, 2, 0, 0, 0, 0, 200, 200), "never written"),
            ((2, 0, 0, 0, 0, 0, 200, 200), "image_index"), ((0, 0, NW - 199, 0, 0, 0, 200, 200), "leaves"),
            ((0, 0, 0, 0, 0, NW - 199, 200, 200), "leaves")]


@pytest.fixture(scope="module")
def refusal_ctx():
    p = _ctx(batch=2)
    assert p.execute(np.stack([phantom(N, 5, noise=4.0), phantom(N, 6, noise=4.0)])), mp.last_error()
    p.sim_capture(0, 1)
    outs = [p.out_pixels(0), p.out_pixels(1)]
    yield p, outs
    p.cleanup()


@pytest.mark.parametrize("case,words", REFUSALS)
def test_refusals_return_0_with_a_message_and_change_nothing(refusal_ctx, case, words):
    p, outs = refusal_ctx
    lib = mp.load_library()
    res = (mp.SimScalesResult * 65)()
    marker = np.frombuffer(res, dtype=np.uint8)
    marker[:] = 0xAB
    good = mp.SimQuery(*GOOD)
    h, count, arr, scales, out = p._h, 2, (mp.SimQuery * 2)(good, good), 5, res
    if case == "ctx":
        h = None
    elif case == "queries":
        arr = None
    elif case == "results":
        out = None
    elif case == "count0":
        count = 0
    elif case == "count65":
        count, arr = 65, (mp.SimQuery * 65)(*([good] * 65))
    elif case == "scales0":
        scales = 0
    elif case == "scales6":
        scales = 6
    else:
        arr = (mp.SimQuery * 2)(good, mp.SimQuery(*case))     # one bad query refuses the call
    assert lib.musica_sim_multiscale(h, count, arr, scales, out) == 0
    msg = mp.last_error()
    assert words in msg and "musica_sim_multiscale" in msg, msg
    assert np.all(marker == 0xAB)                              # nothing was written
    assert np.array_equal(p.sim_get_reference(0), outs[1])
    assert np.array_equal(p.out_pixels(0), outs[0]) and np.array_equal(p.out_pixels(1), outs[1])
    if words == "7 x 7" or case in ("scales0", "scales6"):     # the restatement refuses the same
        with pytest.raises(ValueError):
            z = np.zeros((200, 200) if isinstance(case, str) else (case[7], case[6]), dtype=np.uint8)
            H.multiscale_similarities(z, z, scales)
    # the context still answers
    assert p.sim_multiscale([GOOD], 5)[0]["scales"] == 5


def _close(a, b, what):
    """Two study rows' values: floats to TOL, everything else (ints, None, lists of them, dicts) alike."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), what
        for k in a:
            _close(a[k], b[k], what + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _close(x, y, what + (i,))
    elif isinstance(a, float):
        assert abs(a - b) <= TOL, (what, a, b)
    else:
        assert a == b, (what, a, b)


def test_device_studies_agree_with_the_host_scored_study():
    raw = phantom(N, 11, noise=4.0)
    args = dict(shutters=[200, 225], translations=[60], rotations=[9], sigmas=[], factors=[], symmetries=[4], scales=5)
    runs = {}
    for mode in ("host", "device_metrics", "device_alterations"):
        runner = H.Runner(N, 0, device_metrics=mode == "device_metrics", device_alterations=mode == "device_alterations")
        runs[mode] = H.run_study(raw, runner, rng=np.random.default_rng(5), **args)
        runner.close()
    host = runs["host"]
    assert [r["alteration"] for r in host] == ["unaltered", "c_sh_200", "c_sh_225", "t_x_60", "t_y_60", "r_9", "d4_4"]
    # the collimator crops are 92 and 42 pixels wide: 4 and 3 scales
    assert [r["direct_scales"]["scales"] for r in host] == [5] * 7
    assert [None if r["registered_scales"] is None else r["registered_scales"]["scales"] for r in host][:5] == [None, 4, 3, 5, 5]
    for mode in ("device_metrics", "device_alterations"):
        rows = runs[mode]
        assert [r["alteration"] for r in rows] == [r["alteration"] for r in host]
        for r, h in zip(rows, host):
            if mode == "device_alterations" and r["alteration"].startswith("c_sh_"):
                continue                      # the geometric rows only: the device draws the shutters' noise from its own stream
            for key in ("direct_scales", "registered_scales"):
                _close(r[key], h[key], (mode, r["alteration"], key))
