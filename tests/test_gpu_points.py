"""The point-response pair on the device (kernels_points.hip): musica_alter_points against harness.insert_points and
musica_sim_points against harness.point_statistics, bit for bit (clusters across a tile corner and on a tile's last and first column,
windows flush with the plane's corners, a tile with as many points as pitch 9 allows, the largest list, the rule's edge contrasts, every
store width, the study size; the three kernel forms R = 4, 16, 32, one group and sixteen, empty groups, groups over several chunks and
interleaved, the u32 bound reached), that they repeat and do not depend on the list's order, what they must leave alone, their
refusals, and the point_ rows of a study on its three paths.

Nothing here asserts what a response looks like: the numbers of a point_ row are findings, not premises."""
import csv
import os

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

TOL = 1e-12   # what the similarity tests hold between the device metrics and numpy's
CONTRASTS = (1024, 1023, 512, 1, -1, -1024, -64512)   # the rule's edge values


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _full_range_u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    a[0, -1], a[-1, 0] = 65535, 0
    a[63, 63], a[63, 64], a[64, 63], a[64, 64] = 0, 65535, 1, 1024    # under the clusters across the tile corner
    assert a.min() == 0 and a.max() == 65535
    return a


def _with_contrasts(points, radius=4):
    return tuple((x, y, radius, s, CONTRASTS[i % len(CONTRASTS)], i % mp.POINT_MAX_GROUPS) for i, (x, y, s) in enumerate(points))


def _corner_list(n):
    """For a side n >= 84, R = 4: a 2 x 2 cluster over the four tiles that meet at (63|64, 63|64), a 2 x 2 cluster that ends on the last
    column of tile 0, a 3 x 3 one that starts on the first column of tile 1, a single pixel on that column, and windows flush with the
    four corners of the plane; the rest of the plane has no point."""
    return _with_contrasts([(63, 63, 2), (62, 20, 2), (65, 35, 3), (64, 50, 1), (4, 4, 3), (n - 5, 4, 2), (4, n - 5, 1), (n - 5, n - 5, 3)])


def _packed_list(n):
    """R = 4 points at pitch 9 with centres 9, 18, ..: the cores that meet tile (1, 1) = [64, 128)^2 have their centres in [63, 128],
    eight to an axis, so that tile lists 64 points, what windows of side 9 at pitch 9 allow (the capacity argument admits 67)."""
    centres = range(9, n - 4, 9)
    assert sum(1 for c in centres if 63 <= c <= 128) == 8
    return _with_contrasts([(x, y, 1 + (x + y) % 3) for y in centres for x in centres])


def _largest_list(side):
    """POINT_MAX points, R = 4 at pitch 9, for a plane of at least 576 pixels a side."""
    assert side >= 576
    return tuple((4 + 9 * j, 4 + 9 * i, 4, 1 + (i + j) % 3, CONTRASTS[(i + j) % len(CONTRASTS)], 0) for i in range(64) for j in range(64))


def _check(p, raw, points, image_index=0):
    p.alter_points(points, image_index)
    got = p.input_pixels()[image_index].copy()
    assert np.array_equal(got, H.insert_points(raw, points))
    return got


@pytest.mark.parametrize("n", [84, 88, 90, 137])    # 84 % 8 = 4 and 90 % 8 = 2: 4-byte words; 88: whole 16-byte words; 137: odd, single pixels; the second tile ragged
def test_alter_points_is_bit_identical(n):
    raw = _full_range_u16(n, n)
    p = _ctx(n)
    p.alter_set_source(raw)
    lists = [_corner_list(n), ((63, 63, 4, 3, 1024, 0),), ((63, 63, 4, 2, -64512, 3),)]   # ... and a 3 x 3 and a 2 x 2 cluster alone on the corner
    if n == 137:
        lists.append(_packed_list(n))
    for points in lists:
        got = _check(p, raw, points)
        p.alter_none()
        p.alter_points(points[::-1])                                              # a reversed list gives identical bytes
        assert np.array_equal(p.input_pixels()[0], got)
    for c in CONTRASTS:                                                           # each contrast over the four tiles' corner
        got = _check(p, raw, ((63, 63, 4, 2, c, 0), (n - 7, 20, 4, 3, c, 1)))
        if c == 1024:
            assert not got[63:65, 63:65].any()                                    # a dead cluster
    p.cleanup()


def test_alter_points_with_the_largest_list():
    n = 596
    raw = _full_range_u16(n, 5)
    p = _ctx(n)
    p.alter_set_source(raw)
    points = _largest_list(n)
    assert len(points) == mp.POINT_MAX
    got = _check(p, raw, points)
    p.alter_points(points[::-1])
    assert np.array_equal(p.input_pixels()[0], got)
    p.cleanup()


def test_only_the_named_image_is_written():
    """N^2 odd: image 1 of the input buffer starts on a 2-byte boundary only; the neighbours on both sides keep every pixel."""
    n = 201
    raw = _full_range_u16(n, 2)
    p = _ctx(n, batch=3)
    base = np.stack([_full_range_u16(n, 20 + k) for k in range(3)])
    p.upload(base)
    p.alter_set_source(raw)
    for points in (_corner_list(n), H.point_grid(n, -64512), _packed_list(n)):
        p.alter_points(points, image_index=1)
        got = p.input_pixels()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2])
        assert np.array_equal(got[1], H.insert_points(raw, points))
    p.cleanup()


def test_alter_points_is_bit_identical_at_the_study_size():
    n = 3072
    raw = _full_range_u16(n, 7)
    p = _ctx(n)
    p.alter_set_source(raw)
    points = H.point_grid(n, 1024)
    assert len(points) == 3969
    _check(p, raw, points)
    p.cleanup()


# ---- the measurement -------------------------------------------------------------------------------------------------------------------
N_SIM = 320
NW_SIM = N_SIM - 2 * mp.OUT_MARGIN


def _lattice(radius, group):
    """Windows of half-side `radius` side by side from the top-left corner of the 300-pixel output plane, the last of each row and
    column moved flush with the far side; group(i, j) gives the group of the point in row i, column j."""
    side = 2 * radius + 1
    centres = [radius + side * k for k in range(NW_SIM // side)]
    centres[-1] = NW_SIM - 1 - radius
    return tuple((x, y, radius, 1, 1, group(i, j)) for i, y in enumerate(centres) for j, x in enumerate(centres))


SOME = (0, 3, 7, 15)
LISTS = {
    "r4_one_group": _lattice(4, lambda i, j: 0),                                  # 1089 points: 18 chunks, the last ragged
    "r4_interleaved": _lattice(4, lambda i, j: (33 * i + j) % 2),                  # two groups of 9 chunks each, alternating in list order
    "r4_sixteen": _lattice(4, lambda i, j: (i + 2 * j) % 16),
    "r16_one_group": _lattice(16, lambda i, j: 0),                                # 81 points: two chunks
    "r16_some_of_sixteen": _lattice(16, lambda i, j: SOME[(i + j) % 4]),           # groups 0, 3, 7, 15 of 16: twelve stay empty
    "r16_group_15_only": _lattice(16, lambda i, j: 15),
    "r32_one_group": _lattice(32, lambda i, j: 0),                                # 16 points
    "r32_sixteen": _lattice(32, lambda i, j: 4 * i + j),                           # one point a group
    "r32_one_point": ((NW_SIM - 33, 32, 32, 1, 1, 0),),                            # flush with the top-right corner
    "r5_one_point": ((150, 150, 5, 3, 1, 2),),
}


def _same(got, want):
    assert got["points"] == want["points"]
    assert len(got["groups"]) == len(want["groups"])
    for g, w in zip(got["groups"], want["groups"]):
        assert g["count"] == w["count"]
        for k in mp.POINT_STACKS:
            assert g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), k


def _identities(stats, points):
    for g, stack in enumerate(stats["groups"]):
        mine = [s for p, s in zip(points, stats["points"]) if p[5] == g]
        assert stack["count"] == len(mine)
        assert (int(stack["sum_a"].sum()), int(stack["sum_b"].sum()), int(stack["ssd"].sum())) == \
            (sum(s["win_sum_a"] for s in mine), sum(s["win_sum_b"] for s in mine), sum(s["win_ssd"] for s in mine))


@pytest.fixture(scope="module")
def stepped():
    p = _ctx(N_SIM)
    assert p.execute(phantom(N_SIM, 25, noise=4.0)), mp.last_error()
    out = p.out_pixels().copy()
    out.setflags(write=False)
    yield p, out
    p.cleanup()


def _planes():
    rng = np.random.default_rng(8)
    random = rng.integers(0, 256, (NW_SIM, NW_SIM), dtype=np.uint8)
    random[0, 0], random[-1, -1] = 0, 255
    return {"random": random, "white": np.full((NW_SIM, NW_SIM), 255, np.uint8)}


@pytest.fixture(scope="module")
def references(stepped):
    """point_statistics of every list against both planes, computed once."""
    _, out = stepped
    return {(name, key): H.point_statistics(out, plane, points, 16 if "sixteen" in key else None)
            for name, plane in _planes().items() for key, points in LISTS.items()}


@pytest.mark.parametrize("key", list(LISTS))
@pytest.mark.parametrize("name", ["random", "white"])
def test_sim_points_is_bit_identical(stepped, references, name, key):
    p, out = stepped
    plane = _planes()[name]
    p.sim_set_reference(2, plane)
    points, groups = LISTS[key], 16 if "sixteen" in key else None
    want = references[name, key]
    got = p.sim_points(points, 2, groups)
    _same(got, want)
    _same(p.sim_points(points, 2, groups), got)                                   # called twice: bit-equal
    _identities(got, points)
    back = p.sim_points(points[::-1], 2, groups)                                  # the reversed list: the same tables, the results permuted
    _same(back, dict(want, points=want["points"][::-1]))
    full = p.sim_compare([(0, 2, 0, 0, 0, 0, NW_SIM, NW_SIM)])[0]["sq_diff_sum"]
    assert sum(s["win_ssd"] for s in got["points"]) <= full
    side = 2 * points[0][2] + 1
    for (x, y, r, _, _, _), s in zip(points[:8], got["points"]):                  # win_ssd is the compare call's integer over the same region
        res = p.sim_compare([(0, 2, x - r, y - r, x - r, y - r, side, side)])[0]
        assert s["win_ssd"] == res["sq_diff_sum"] and s["win_pixels"] == res["pixels"] == side * side
    assert all(type(v) is int for v in got["points"][0].values()) and type(got["groups"][0]["count"]) is int
    if key == "r16_some_of_sixteen":
        assert [g["count"] > 0 for g in got["groups"]] == [k in SOME for k in range(16)]
        assert not any(got["groups"][1][k].any() for k in mp.POINT_STACKS)         # a group without points is all zero


def _set_out(p, values, image_index=0):
    """Makes the 8-bit output of an image `values` ((N, N) integers 0 .. 255; the margin is cropped): graded = (v + 0.5) / 255."""
    p.set_image(mp.IMG_GRADED, 0, ((np.asarray(values) + 0.5) / 255.0).astype(np.float32), image_index=image_index)


def test_sim_points_with_the_largest_group_and_at_the_u32_bound():
    n = 596
    nw = n - 2 * mp.OUT_MARGIN
    p = _ctx(n)
    points = _largest_list(nw)
    values = np.random.default_rng(3).integers(0, 256, (n, n), dtype=np.uint8)
    _set_out(p, values)
    out = p.out_pixels()
    assert np.array_equal(out, values[mp.OUT_MARGIN:-mp.OUT_MARGIN, mp.OUT_MARGIN:-mp.OUT_MARGIN])
    plane = np.random.default_rng(4).integers(0, 256, (nw, nw), dtype=np.uint8)
    white = np.full((nw, nw), 255, np.uint8)
    p.sim_set_reference(0, plane)
    p.sim_set_reference(1, white)
    got = p.sim_points(points, 0)
    _same(got, H.point_statistics(out, plane, points))
    _identities(got, points)
    # an all-zero output against the all-255 slot: every word of the stack is at the bound the u32 accumulators are sized for
    _set_out(p, np.zeros((n, n), np.uint8))
    assert not p.out_pixels().any()
    got = p.sim_points(points, 1)
    stack = got["groups"][0]
    assert stack["count"] == mp.POINT_MAX == 4096
    assert (stack["ssd"] == 4096 * 65025).all() and (stack["sum_b"] == 4096 * 255).all() and not stack["sum_a"].any()
    assert all(s["win_ssd"] == 81 * 65025 and s["core_sum_b"] == 9 * 255 for s in got["points"])
    # the output against itself: every third word is 0
    _set_out(p, values)
    p.sim_capture(2)
    got = p.sim_points(points, 2)
    assert not got["groups"][0]["ssd"].any() and np.array_equal(got["groups"][0]["sum_a"], got["groups"][0]["sum_b"])
    assert all(s["win_ssd"] == 0 and s["core_sum_a"] == s["core_sum_b"] for s in got["points"])
    p.cleanup()


def test_sim_points_reads_the_named_image():
    n = 137
    nw = n - 2 * mp.OUT_MARGIN
    p = _ctx(n, batch=3)
    assert p.execute(np.stack([phantom(n, 30 + k, noise=4.0) for k in range(3)])), mp.last_error()
    plane = np.random.default_rng(1).integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(5, plane)
    points = ((20, 20, 20, 1, 1, 0), (nw - 21, 20, 20, 2, 1, 1), (20, nw - 21, 20, 3, 1, 0))   # an odd plane side, windows flush with three corners
    for k in range(3):
        _same(p.sim_points(points, 5, image_index=k), H.point_statistics(p.out_pixels(k), plane, points))
    p.cleanup()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _array(points):
    return (mp.Defect * len(points))(*[mp.Defect(*d) for d in points])


def test_refusals_leave_the_context_usable():
    n, levels = 264, 4
    nw = n - 2 * mp.OUT_MARGIN
    raw = phantom(n, 25, noise=4.0)
    p = _ctx(n, levels)
    lib = mp.load_library()
    assert p.execute(raw)
    p.sim_capture(0)
    p.alter_set_source(raw)
    p.alter_none()
    graded, slot0, inp = p.graded().copy(), p.sim_get_reference(0), p.input_pixels().copy()
    res = (mp.SimPointResult * mp.POINT_MAX)()
    words = 16 * 3 * 65 * 65
    tables = np.zeros(words, dtype=np.uint32)
    tp = tables.ctypes.data_as(mp._U32P)
    ok = ((40, 40, 6, 2, 512, 0), (100, 40, 6, 3, -1024, 1))

    def refused(rc, text):
        assert rc == 0
        msg = mp.last_error()
        assert text in msg, msg

    def sim(arr, count, groups=2, results=res, t=tp, w=words, idx=0, slot=0, ctx=p):
        return lib.musica_sim_points(ctx._h if ctx else None, idx, slot, count, arr, groups, results, t, w)

    def both(points, text, plane=None, count=None):
        """The list is refused by both entry points (for the measurement in the output plane's coordinates when `plane` is its side)."""
        arr, count = _array(points), len(points) if count is None else count
        if plane in (None, n):
            refused(lib.musica_alter_points(p._h, 0, count, arr), text)
        if plane in (None, nw):
            refused(sim(arr, count), text)

    both(ok, "count", count=0)
    both(ok, "count", count=mp.POINT_MAX + 1)
    for r in (0, 3, 33, 1 << 20):
        both(((130, 130, r, 1, 8, 0),), "radius")
    both(((40, 40, 6, 1, 8, 0), (100, 100, 7, 1, 8, 0)), "radius")                # every point of a list has the same radius
    for s in (0, 4, 1 << 20):
        both(((40, 40, 6, s, 8, 0),), "size")
    for c in (0, 1025, -64513):
        refused(lib.musica_alter_points(p._h, 0, 1, _array(((40, 40, 6, 1, c, 0),))), "contrast")
    assert sim(_array(((40, 40, 6, 1, 0, 0),)), 1) == 1                           # the measurement does not look at it
    both(((40, 40, 6, 1, 8, 16),), "group")                                       # beyond MUSICA_POINT_MAX_GROUPS
    refused(sim(_array(((40, 40, 6, 1, 8, 2),)), 1, groups=2), "group")           # ... and not below the call's groups
    for g in (0, 17):
        refused(sim(_array(ok), 2, groups=g), "groups")
    for d in ((5, 40, 6, 1, 8, 0), (40, 5, 6, 1, 8, 0), (-5, 40, 6, 1, 8, 0), (40, -5, 6, 1, 8, 0)):   # a window one pixel (or more) outside on the near sides
        both((d,), "leaves")
    for side in (n, nw):                                                          # ... and on the far sides of each plane
        both(((side - 6, 40, 6, 1, 8, 0),), "leaves", plane=side)
        both(((40, side - 6, 6, 1, 8, 0),), "leaves", plane=side)
    assert sim(_array(((nw - 7, nw - 7, 6, 1, 8, 0),)), 1) == 1                   # flush is inside
    both(((40, 40, 6, 1, 8, 0), (52, 40, 6, 1, 8, 0)), "disjoint")                # two windows sharing a column
    both(((40, 40, 6, 1, 8, 0), (52, 52, 6, 1, 8, 0)), "disjoint")
    both(((40, 40, 6, 1, 8, 0), (100, 100, 6, 1, 8, 0), (40, 40, 6, 1, 8, 0)), "disjoint")   # the same point twice
    assert sim(_array(((40, 40, 6, 1, 8, 0), (53, 40, 6, 1, 8, 0))), 2) == 1      # side by side is disjoint
    refused(lib.musica_alter_points(None, 0, 2, _array(ok)), "NULL")
    refused(lib.musica_alter_points(p._h, 0, 2, None), "NULL")
    refused(sim(_array(ok), 2, ctx=None), "NULL")
    refused(sim(None, 2), "NULL")
    refused(sim(_array(ok), 2, results=None), "NULL")
    refused(sim(_array(ok), 2, t=None), "NULL")
    refused(sim(_array(ok), 2, w=2 * 3 * 13 * 13 - 1), "table_words")
    assert sim(_array(ok), 2, w=2 * 3 * 13 * 13) == 1
    refused(lib.musica_alter_points(p._h, 1, 2, _array(ok)), "image_index")       # image_index == batch
    refused(lib.musica_alter_points(p._h, 1, 1, _array(((130, 130, 0, 1, 8, 0),))), "radius")   # a bad list AND a bad index: every alteration names its own arguments first
    refused(sim(_array(ok), 2, idx=1), "image_index")
    refused(sim(_array(ok), 2, slot=5), "never written")
    refused(sim(_array(ok), 2, slot=mp.SIM_SLOTS), "slot")
    bad_lists = (((40, 40, 3, 1, 8, 0),), ((40, 40, 6, 1, 8, 0), (100, 100, 7, 1, 8, 0)), ((40, 40, 6, 4, 8, 0),), ((40, 40, 6, 1, 8, 16),),
                 ((40, 40, 6, 1, 8, 0), (52, 40, 6, 1, 8, 0)), ((5, 40, 6, 1, 8, 0),), ())
    for bad in bad_lists:                                                         # the binding refuses before the library
        with pytest.raises(ValueError):
            p.alter_points(bad)
        with pytest.raises(ValueError):
            p.sim_points(bad, 0)
    for c in (0, 1025, -64513):
        with pytest.raises(ValueError):
            p.alter_points(((40, 40, 6, 1, c, 0),))
    for groups in (0, 17, 1):                                                     # 1: the list has a point in group 1
        with pytest.raises(ValueError):
            p.sim_points(ok, 0, groups)
    fresh = _ctx(n, levels)
    refused(lib.musica_alter_points(fresh._h, 0, 2, _array(ok)), "no source")
    refused(sim(_array(ok), 2, ctx=fresh), "never written")
    small = _ctx(2 * mp.OUT_MARGIN)
    refused(sim(_array(ok), 2, ctx=small), "margin")
    small.cleanup()
    # nothing was touched by the refused calls (nor by the measurements that ran): no image, no result, no slot; slot 1 is unwritten
    assert np.array_equal(p.input_pixels(), inp) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    with pytest.raises(RuntimeError):
        p.sim_get_reference(1)
    # a successful insertion changes neither the last step's results nor a slot ...
    p.alter_points(ok)
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    assert not p.sim_points(H.output_points(((60, 60, 6, 1, 8, 0),)), 0)["groups"][0]["ssd"].any()   # the output is still the captured one
    # ... and the step on the resident buffer processes what the insertion wrote
    assert p.execute_device()
    p.sync()
    assert fresh.execute(H.insert_points(raw, ok))
    assert np.array_equal(p.graded(), fresh.graded())
    assert np.array_equal(p.input_pixels()[0], H.insert_points(raw, ok))
    _same(p.sim_points(H.output_points(ok), 0), H.point_statistics(fresh.out_pixels(), slot0, H.output_points(ok)))
    p.cleanup()
    fresh.cleanup()


# ---- the study -------------------------------------------------------------------------------------------------------------------------
def _grids(n):
    return dict(shutters=H.scaled(H.SHUTTERS, n)[:1], translations=H.scaled(H.TRANSLATIONS, n)[:1], rotations=[9], sigmas=[16.0], factors=[0.05])


def _study(n, points, **runner_args):
    runner = H.Runner(n, 0, **runner_args)
    rows = H.run_study(phantom(n, 11, noise=4.0), runner, rng=np.random.default_rng(5), scatters=[(3, 1, 2)], points=points,
                       point_tables=points is not None, **_grids(n))
    runner.close()
    return rows


def test_study_rows_agree_on_the_three_paths():
    n = 201
    grids = H.POINTS(n)
    studies = {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = _study(n, grids, **args)
        plain = _study(n, None, **args)
        assert [r["alteration"] for r in rows[len(plain):]] == ["point_%d" % c for c in H.POINT_CONTRASTS], name
        # the rows before them are the rows of the study without points, but for the key
        assert all(r["points"] is None for r in rows[:len(plain)]), name
        assert [{k: v for k, v in r.items() if k != "points"} for r in rows[:len(plain)]] == plain, name
        assert all("points" not in r for r in plain), name
        studies[name] = rows[len(plain):]
        for r in studies[name]:
            assert set(r) == {"alteration", "mean_cnr", "direct", "registered", "points"} and r["registered"] is None, (name, r["alteration"])
            d = r["points"]
            assert [g["count"] for g in d["groups"]] == [3, 3, 3] and d["all"]["count"] == 9 and len(d["per_point"]) == 9 and len(d["stacks"]) == 3
    assert studies["alterations"] == studies["metrics"]   # every number of every row, exactly
    for h, d in zip(studies["host"], studies["metrics"]):
        assert h["alteration"] == d["alteration"] and h["mean_cnr"] == d["mean_cnr"]
        assert h["points"] == d["points"], h["alteration"]                        # exact integers, one summary: equal to the last bit
        for k in mp.SIM_METRICS:
            assert abs(h["direct"][k] - d["direct"][k]) <= TOL, (h["alteration"], k, h["direct"][k], d["direct"][k])


def test_cli_points_writes_the_rows(tmp_path):
    out = str(tmp_path / "out")
    assert H.main(["--device-alterations", "--points", "--size", "512", "--levels", "5", "--out", out]) == 0
    names = ["point_%d" % c for c in H.POINT_CONTRASTS]
    direct = list(csv.reader(open(os.path.join(out, "direct_robustness.csv"))))
    reg = list(csv.reader(open(os.path.join(out, "reg_based_robustness.csv"))))
    assert [r[1] for r in direct[-5:]] == names and not any(r[1].startswith("point_") for r in reg)
    assert len(direct) == 1 + 30 + 5
    lines = list(csv.reader(open(os.path.join(out, "point_response.csv"))))
    grid = H.point_grid(512, 1024)
    assert lines[0] == H.POINT_CSV_HEADER and [(l[1], l[2]) for l in lines[1:]] == [(name, g) for name in names for g in ("0", "1", "2", "all")]
    assert all(int(l[3]) == (len(grid) if l[2] == "all" else len(grid) // 3) for l in lines[1:])
    plain = str(tmp_path / "plain")
    assert H.main(["--device-alterations", "--size", "512", "--levels", "5", "--out", plain]) == 0
    assert not os.path.exists(os.path.join(plain, "point_response.csv"))
    assert open(os.path.join(plain, "direct_robustness.csv")).read() == "".join(open(os.path.join(out, "direct_robustness.csv")).readlines()[:31])
