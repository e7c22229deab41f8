"""Exact block matching on the device (musica_sim_displace; kernels_displace.hip) against harness.py's restatement: the tables and the
tile tables entry for entry, the zero shift against musica_sim_compare, the refusals, what the call leaves untouched, and a device
study with displacement=4 against the host-metric one, floats included."""
import ctypes as C
import itertools

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

U64P = C.POINTER(C.c_uint64)
U32P = C.POINTER(C.c_uint32)


def _ctx(n, levels=4, batch=1, flags=0):
    p = mp.MusicaProcessing()
    assert p.init(n, levels=levels, batch=batch, flags=flags | mp.FLAG_NO_AUTOTUNE), mp.last_error()
    return p


def _set_out(p, i, values):
    """Makes the 8-bit output of image i `values` ((N, N) integers 0 .. 255; the margin is cropped): graded = (v + 0.5) / 255."""
    p.set_image(mp.IMG_GRADED, 0, ((np.asarray(values) + 0.5) / 255.0).astype(np.float32), image_index=i)


def _textured(rng, n, smooth=3):
    """Random u8 texture with some correlation between neighbours, so that shifts have a clear best match."""
    v = rng.integers(0, 256, size=(n + smooth, n + smooth)).astype(np.int64)
    acc = sum(v[i:i + n, j:j + n] for i in range(smooth) for j in range(smooth)) // (smooth * smooth)
    return np.clip(acc + rng.integers(-9, 10, size=(n, n)), 0, 255)


def _check(p, queries, radius, outs, slots, compare=True):
    """One call with tables and tile tables against the restatement, query by query; returns the results."""
    res = p.sim_displace(queries, radius, tables=True, tiles=True)
    assert len(res) == len(queries)
    cmp_res = p.sim_compare(queries) if compare else [None] * len(queries)
    s = 2 * radius + 1
    for r, c, q in zip(res, cmp_res, queries):
        i, slot = q[0], q[1]
        region = tuple(q[2:])
        w, h = region[4], region[5]
        tt = H.displacement_tile_tables(outs[i], slots[slot], region, radius)
        T = H.displacement_table(outs[i], slots[slot], region, radius)
        assert r["tile_tables"].dtype == np.uint32 and r["tile_tables"].shape == tt.shape == ((h + 63) // 64, (w + 63) // 64, s, s), q
        assert np.array_equal(r["tile_tables"], tt), q
        assert r["table"].dtype == np.uint64 and r["table"].shape == (s, s)
        assert np.array_equal(r["table"].astype(np.int64), T), q
        d = H.displacement_from_table(T)
        assert (r["dx"], r["dy"], r["ssd_min"], r["ssd_zero"]) == (d["dx"], d["dy"], d["ssd_min"], d["ssd_zero"]), q
        assert H.displacement_from_table(r["table"]) == d
        assert (r["pixels"], r["tiles_x"], r["tiles_y"]) == (w * h, tt.shape[1], tt.shape[0]), q
        assert r["tiles_off"] == H.displacement_tiles_off(tt), q
        if c is not None:
            assert r["ssd_zero"] == c["sq_diff_sum"] and r["pixels"] == c["pixels"], q
    plain = p.sim_displace(queries, radius)
    for a, b in zip(plain, res):
        assert "table" not in a and "tile_tables" not in a and all(a[k] == b[k] for k in a)
    return res


def _identical(x, y):
    assert len(x) == len(y)
    for a, b in zip(x, y):
        assert set(a) == set(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
            else:
                assert a[k] == b[k], k


@pytest.mark.parametrize("n", [96, 136, 520])
def test_tables_equal_the_restatement_at_ragged_sides(n):
    nw = n - 2 * mp.OUT_MARGIN
    rng = np.random.default_rng(n)
    p = _ctx(n)
    v = _textured(rng, n)
    _set_out(p, 0, v)
    out = p.out_pixels(0)
    assert np.array_equal(out, v[10:-10, 10:-10])
    ref = rng.integers(0, 256, size=(nw, nw), dtype=np.uint8)
    moved = np.roll(out, (2, -3), axis=(0, 1))             # moved[y][x] = out[y - 2][x + 3]: out matches it at dx = -3, dy = 2
    p.sim_set_reference(0, ref)
    p.sim_set_reference(3, moved)
    slots = {0: ref, 3: moved}
    for radius in (1, 3, 8, 16):
        room = nw - 2 * radius                               # at least 44
        # every residue of ax, bx and w mod 4: 64 queries in one launch, the offsets within the play the widths leave
        queries = []
        for ra, rb, rw in itertools.product(range(4), repeat=3):
            w = room - 3 - (room - 3 - rw) % 4               # the widest width of that residue that leaves bx three columns of play
            h = (room if radius < 8 else min(room, 67)) - (ra + rb + rw) % 5   # low regions at the large radii: the host's S^2 crops
            queries.append((0, (0, 3)[(ra + rw) % 2], ra, (3 * ra) % (nw - h + 1), radius + rb, radius + rb % (room - h + 1), w, h))
        assert {(q[2] % 4, q[4] % 4, q[6] % 4) for q in queries} == set(itertools.product(range(4), repeat=3))
        res = _check(p, queries, radius, [out], slots)
        # the planted shift, over the part of the frame the roll did not wrap (and the radius leaves)
        if radius >= 3 and room - 6 >= 7:
            q = (0, 3, radius + 3, radius + 3, radius + 3, radius + 3, room - 6, room - 6)
            r = _check(p, [q], radius, [out], slots)[0]
            assert (r["dx"], r["dy"], r["ssd_min"]) == (-3, 2, 0)
            assert r["tiles_off"] == r["tiles_x"] * r["tiles_y"]
        assert len(res) == 64
    p.cleanup()


def test_many_queries_batches_and_every_way_to_write_a_slot():
    n, batch = 520, 3
    nw = n - 2 * mp.OUT_MARGIN
    rng = np.random.default_rng(21)
    p = _ctx(n, batch=batch)
    vals = [_textured(rng, n), rng.integers(0, 256, size=(n, n)), _textured(rng, n, 5)]
    for i, v in enumerate(vals):
        _set_out(p, i, v)
    outs = [p.out_pixels(i) for i in range(batch)]
    for i, v in enumerate(vals):
        assert np.array_equal(outs[i], v[10:-10, 10:-10])
    host = rng.integers(0, 256, size=(nw, nw), dtype=np.uint8)
    p.sim_capture(0, 2)                                    # slot 0: image 2's output
    p.sim_set_reference(1, host)
    p.sim_transform_reference(2, 0, 5)                     # slot 2: a flip of slot 0
    slots = {0: outs[2], 1: host, 2: H.apply_symmetry(outs[2], 5)}
    for s, v in slots.items():
        assert np.array_equal(p.sim_get_reference(s), v)
    # 64 queries of different sizes in one call, image_index 2 among them, all three slots
    radius = 3
    queries = [(i % 3, i % 3 if i % 5 else (i + 1) % 3, i, 2 * i % 50, radius + 3 * i % 40, radius + i, nw - 2 * radius - 5 * i, nw - 2 * radius - 3 * i - 40 * (i % 4))
               for i in range(64)]
    first = _check(p, queries, radius, outs, slots)
    _identical(first, p.sim_displace(queries, radius, tables=True, tiles=True))        # byte-identical from call to call
    # image 2 against its own capture: zero on the diagonal of no shift, in every tile
    r = _check(p, [(2, 0, 8, 8, 8, 8, nw - 16, nw - 16)], 8, outs, slots)[0]
    assert r["ssd_zero"] == r["ssd_min"] == 0 and (r["dx"], r["dy"], r["tiles_off"]) == (0, 0, 0)
    assert np.all(r["tile_tables"][:, :, 8, 8] == 0)
    # a smaller call after a larger one, a larger radius after a smaller one: the tile-table buffer is regrown, not reused too small
    _check(p, [(1, 1, 16, 16, 16, 16, 100, 71)], 16, outs, slots)
    _check(p, [(0, 2, 16, 16, 16, 16, nw - 32, nw - 32), (1, 1, 0, 0, 16, 16, 7, 7)], 16, outs, slots)
    p.cleanup()


def test_extremes():
    n = 64 * 5 + 2 * 16 + 20                                # room for 5 x 4 whole tiles at radius 16
    nw = n - 2 * mp.OUT_MARGIN
    rng = np.random.default_rng(2)
    p = _ctx(n, levels=0)
    _set_out(p, 0, np.full((n, n), 255))
    assert np.all(p.out_pixels(0) == 255)
    p.sim_set_reference(0, np.zeros((nw, nw), dtype=np.uint8))
    tile, total = 64 * 64 * 65025, 20 * 64 * 64 * 65025
    assert tile < 2 ** 32 < total                           # a tile entry fits u32, the sum of the 20 tiles does not
    for radius in (16, 1):
        r = p.sim_displace([(0, 0, 16, 16, 16, 16, 320, 256)], radius, tables=True, tiles=True)[0]
        assert r["tile_tables"].shape == (4, 5, 2 * radius + 1, 2 * radius + 1)
        assert np.all(r["tile_tables"] == tile)
        assert np.all(r["table"] == total)
        assert (r["dx"], r["dy"], r["tiles_off"], r["ssd_zero"], r["ssd_min"]) == (0, 0, 0, total, total)
    v = rng.integers(0, 256, size=(n, n))
    _set_out(p, 0, v)
    p.sim_capture(1, 0)
    r = _check(p, [(0, 1, 16, 16, 16, 16, 320, 256), (0, 1, 5, 5, 5, 5, nw - 10, nw - 10)], 5, [p.out_pixels(0)], {1: p.out_pixels(0)})
    for x in r:
        assert x["ssd_zero"] == 0 and (x["dx"], x["dy"], x["tiles_off"]) == (0, 0, 0) and np.all(x["tile_tables"][:, :, 5, 5] == 0)
    p.cleanup()


def test_full_size_frame():
    n, radius = 3072, 2
    nw = n - 2 * mp.OUT_MARGIN
    rng = np.random.default_rng(30)
    p = _ctx(n, levels=0)
    v = np.clip(np.add.outer(np.arange(n), np.arange(n)) // 32 + rng.integers(-30, 31, size=(n, n)), 0, 255)
    _set_out(p, 0, v)
    out = p.out_pixels(0)
    assert np.array_equal(out, v[10:-10, 10:-10])
    ref = np.clip(np.roll(out, 1, axis=1).astype(np.int32) + rng.integers(-4, 5, size=(nw, nw)), 0, 255).astype(np.uint8)
    p.sim_set_reference(0, ref)
    q = (0, 0, radius, radius, radius, radius, nw - 2 * radius, nw - 2 * radius)
    r = _check(p, [q], radius, [out], {0: ref})[0]
    assert (r["tiles_x"], r["tiles_y"]) == (48, 48) and r["pixels"] == (nw - 4) ** 2
    assert (r["dx"], r["dy"]) == (1, 0)
    _identical([r], p.sim_displace([q], radius, tables=True, tiles=True))
    p.cleanup()


def test_the_call_changes_nothing():
    n = 276
    nw = n - 2 * mp.OUT_MARGIN
    px = np.stack([phantom(n, 5, noise=4.0), phantom(n, 6, noise=4.0)])
    p = _ctx(n, levels=0, batch=2)
    assert p.execute(px), mp.last_error()
    outs = [p.out_pixels(0), p.out_pixels(1)]
    p.sim_capture(0, 1)
    rng = np.random.default_rng(1)
    other = rng.integers(0, 256, size=(nw, nw), dtype=np.uint8)
    p.sim_set_reference(5, other)
    queries = [(0, 0, 4, 4, 4, 4, nw - 8, nw - 8), (1, 5, 0, 0, 4, 4, 100, 99)]
    a = _check(p, queries, 4, outs, {0: outs[1], 5: other})
    b = p.sim_displace(queries, 4, tables=True, tiles=True)
    _identical(a, b)
    assert np.array_equal(p.sim_get_reference(0), outs[1]) and np.array_equal(p.sim_get_reference(5), other)
    assert np.array_equal(p.out_pixels(0), outs[0]) and np.array_equal(p.out_pixels(1), outs[1])
    assert p.execute(px), mp.last_error()
    assert np.array_equal(p.out_pixels(0), outs[0]) and np.array_equal(p.out_pixels(1), outs[1])
    p.cleanup()


_N = 276
_NW = _N - 2 * mp.OUT_MARGIN
_R = 4
_GOOD = (0, 0, 0, 0, _R, _R, _NW - 2 * _R, _NW - 2 * _R)      # the grown b window touches all four edges
BAD_QUERIES = [((0, mp.SIM_SLOTS) + _GOOD[2:], "slot"), ((0, 6) + _GOOD[2:], "never written"), ((2, 0) + _GOOD[2:], "batch"),
               ((0, 0, 0, 0, _R, _R, 6, 50), "7 x 7"), ((0, 0, 0, 0, _R, _R, 50, 6), "7 x 7"),
               ((0, 0, _NW - 49, 0, _R, _R, 50, 50), "leaves"), ((0, 0, 0, _NW - 49, _R, _R, 50, 50), "leaves"),      # the a region
               ((0, 0, 0, 0, _R + 1, _R, _NW - 2 * _R, _NW - 2 * _R), "grown"), ((0, 0, 0, 0, _R, _R + 1, _NW - 2 * _R, _NW - 2 * _R), "grown"),
               ((0, 0, 0, 0, _R - 1, _R, 50, 50), "grown"), ((0, 0, 0, 0, _R, _R - 1, 50, 50), "grown"),
               ((0, 0, 0, 0, _NW - 50 - _R + 1, _R, 50, 50), "grown"), ((0, 0, 0, 0, _R, _NW - 50 - _R + 1, 50, 50), "grown"),
               ((0, 0, 0, 0, 0xFFFFFFF0, _R, 32, 32), "leaves")]


@pytest.fixture(scope="module")
def refusal_ctx():
    p = _ctx(_N, levels=0, batch=2)
    px = np.stack([phantom(_N, 5, noise=4.0), phantom(_N, 6, noise=4.0)])
    assert p.execute(px), mp.last_error()
    p.sim_capture(0, 1)
    yield p
    p.cleanup()


def _refused(p, count, arr, radius, res, words, tab=None, tiles=None):
    lib = mp.load_library()
    assert lib.musica_sim_displace(p._h if p is not None else None, count, arr, radius, res, tab, tiles) == 0
    msg = mp.last_error()
    assert words in msg and "musica_sim_displace" in msg, msg


@pytest.mark.parametrize("case", ["ctx", "queries", "results", "count0", "count65", "radius0", "radius17"])
def test_refuses_bad_arguments(refusal_ctx, case):
    p = refusal_ctx
    q = mp.SimQuery(*_GOOD)
    res = (mp.SimDisplaceResult * 65)()
    one = (mp.SimQuery * 1)(q)
    if case == "ctx":
        _refused(None, 1, one, _R, res, "NULL")
    elif case == "queries":
        _refused(p, 1, None, _R, res, "NULL")
    elif case == "results":
        _refused(p, 1, one, _R, None, "NULL")
    elif case == "count0":
        _refused(p, 0, one, _R, res, "count")
    elif case == "count65":
        _refused(p, 65, (mp.SimQuery * 65)(*([q] * 65)), _R, res, "count")
    elif case == "radius0":
        _refused(p, 1, (mp.SimQuery * 1)(mp.SimQuery(0, 0, 0, 0, 20, 20, 50, 50)), 0, res, "radius")
    else:
        _refused(p, 1, (mp.SimQuery * 1)(mp.SimQuery(0, 0, 0, 0, 20, 20, 50, 50)), 17, res, "radius")


@pytest.mark.parametrize("bad,words", BAD_QUERIES)
def test_refuses_bad_queries_before_any_device_work(refusal_ctx, bad, words):
    p = refusal_ctx
    s2 = (2 * _R + 1) ** 2
    res = (mp.SimDisplaceResult * 2)()
    tab = np.full(2 * s2, 0xABCD, dtype=np.uint64)
    tiles = np.full(2 * 25 * s2, 0xABCD, dtype=np.uint32)
    arr = (mp.SimQuery * 2)(mp.SimQuery(*_GOOD), mp.SimQuery(*bad))          # one bad query refuses the call
    _refused(p, 2, arr, _R, res, words, tab.ctypes.data_as(U64P), tiles.ctypes.data_as(U32P))
    assert np.all(tab == 0xABCD) and np.all(tiles == 0xABCD)               # nothing was written
    if words in ("7 x 7", "leaves", "grown"):                              # the restatement refuses the same geometry
        with pytest.raises(ValueError):
            H.displacement_table(np.zeros((_NW, _NW), np.uint8), np.zeros((_NW, _NW), np.uint8), bad[2:], _R)


def test_accepts_a_window_that_touches_the_edges(refusal_ctx):
    p = refusal_ctx
    outs = [p.out_pixels(0), p.out_pixels(1)]
    _check(p, [_GOOD, (1, 0, _NW - 50, _NW - 50, _NW - 50 - _R, _NW - 50 - _R, 50, 50), (0, 0, 0, 0, _R, _R, 7, 7)], _R, outs, {0: outs[1]})


SHIFT_ROWS = ("t_x_", "t_y_", "d4_")


def test_study_with_displacement_on_the_device_equals_the_host():
    n, levels, radius = 520, 5, 4
    raw = phantom(n, 11, noise=4.0)
    args = dict(shutters=H.scaled(H.SHUTTERS, n)[:2], translations=H.scaled(H.TRANSLATIONS, n)[:2], rotations=[9, 45], sigmas=[16.0],
                factors=[0.05], symmetries=H.SYMMETRIES, displacement=radius)
    studies = {}
    for name, kw in (("host", {}), ("metrics", {"device_metrics": True}), ("alterations", {"device_alterations": True})):
        runner = H.Runner(n, levels, **kw)
        studies[name] = H.run_study(raw, runner, rng=np.random.default_rng(5), **args)
        runner.close()
    host, metrics, alterations = studies["host"], studies["metrics"], studies["alterations"]
    assert [r["alteration"] for r in host] == [r["alteration"] for r in metrics] == [r["alteration"] for r in alterations]
    geometric = lambda r: not r["alteration"].startswith(("c_sh_", "gn_", "pn_"))   # the noise rows draw from different streams
    for h, m, a in zip(host, metrics, alterations):
        for key in ("direct_shift", "registered_shift"):
            assert key in h and key in m and key in a
            assert h[key] == m[key], (h["alteration"], key, h[key], m[key])          # exact integer tables, one summary: floats included
            if geometric(h):
                assert m[key] == a[key], (h["alteration"], key, m[key], a[key])
        assert (h["registered_shift"] is None) == (h["registered"] is None)
        print(h["alteration"], "direct", {k: h["direct_shift"][k] for k in ("dx", "dy", "sub_dx", "sub_dy", "tiles_off", "tiles")},
              "registered", h["registered_shift"] and {k: h["registered_shift"][k] for k in ("dx", "dy", "sub_dx", "sub_dy", "tiles_off", "tiles")})
    assert host[0]["direct_shift"]["dx"] == host[0]["direct_shift"]["dy"] == 0 and host[0]["direct_shift"]["mse_at_zero"] == 1.0
    for r in metrics:
        if r["alteration"].startswith(SHIFT_ROWS):
            g = r["registered_shift"]
            assert g is not None and g["dx"] == 0 and g["dy"] == 0, (r["alteration"], g)
    # without the option the device study's rows are those rows less the two keys
    runner = H.Runner(n, levels, device_metrics=True)
    plain = H.run_study(raw, runner, rng=np.random.default_rng(5), **{k: v for k, v in args.items() if k != "displacement"})
    runner.close()
    assert plain == [{k: v for k, v in r.items() if k not in ("direct_shift", "registered_shift")} for r in metrics]
