"""The texture metric on the device: musica_sim_cooccurrence against metrics.cooccurrence_statistics, word for word, at every number of
levels and at distance lists that hold the smallest and the largest distance; regions of one pixel, as wide or as high as a distance and
one more, of exactly one tile, of four tiles whose pairs cross the tile corner in every direction, of several tiles with ragged ends
and the full frame, where the halo meets the plane's edge; one and four queries a call, one of them without a pair; workgroups that
take several tiles; contents that put the counts in known cells and on the level boundaries; a flat plane that puts a whole region's
pairs in one counter; the marginals against the device's own joint histogram; that results repeat; what the call must leave alone and
its refusals; a study's *_texture keys on its three paths. Everything compared is an integer: no tolerance anywhere."""
import functools

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

_U32P = mp.C.POINTER(mp.C.c_uint32)
M = mp.OUT_MARGIN
N_SIM = 320
NW = N_SIM - 2 * M
FULL = (0, 0, 0, 0, NW, NW)
LEVELS = (8, 16, 32, 64)
DISTANCES = ((1,), (16,), (1, 2, 4, 8), (3, 5, 16))
OUT = np.random.default_rng(28).integers(0, 256, (NW, NW), dtype=np.uint8)
PLANE = np.random.default_rng(29).integers(0, 256, (NW, NW), dtype=np.uint8)


def shapes(ds):
    """(ax, ay, bx, by, w, h), each the smallest at which one thing can break, for the smallest and the largest distance of a list. The
    origins are odd and differ between the sides, so that no load is 4-byte aligned."""
    out = [(1, 3, 4, 1, 1, 1)]                                                    # one pixel: no pair at all
    for d in sorted({ds[0], ds[-1]}):
        out += [(3, 1, 1, 2, d, 40), (3, 1, 1, 2, d + 1, 40),                     # no horizontal or diagonal pair; one column of them
                (1, 5, 2, 3, 40, d), (1, 5, 2, 3, 40, d + 1)]                     # no vertical or diagonal pair; one row of them
    return out + [(5, 7, 2, 1, 64, 64),                                           # exactly one tile: the halo is all outside the region
                  (7, 5, 1, 3, 65, 65),                                           # four tiles: pairs cross the tile corner in every direction
                  (9, 3, 6, 11, 200, 136),                                        # 4 x 3 tiles with ragged ends of 8
                  FULL]                                                           # 5 x 5 tiles; the halo meets the plane's edge


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _set_out(p, values, image_index=0):
    """Makes the 8-bit output of an image `values` ((N, N) integers 0 .. 255; the margin is cropped): graded = (v + 0.5) / 255."""
    p.set_image(mp.IMG_GRADED, 0, ((np.asarray(values) + 0.5) / 255.0).astype(np.float32), image_index=image_index)
    out = p.out_pixels(image_index)
    assert np.array_equal(out, np.asarray(values)[M:-M, M:-M])
    return out


def _queries(regions, slot, image_index=0):
    return [(image_index, slot) + tuple(r) for r in regions]


def _same(got, want, regions, G, ds, what=None):
    assert len(got) == len(want) == len(regions)
    for g, w, r in zip(got, want, regions):
        assert set(g) == {"table", "pairs"}, what
        assert g["table"].dtype == np.uint32 and g["table"].shape == (len(ds), 4, 2, G, G)
        assert g["pairs"].dtype == np.uint64 and g["pairs"].shape == (len(ds), 4)
        assert np.array_equal(g["pairs"], w["pairs"]), (what, G, ds, r)
        assert np.array_equal(g["table"], w["table"]), (what, G, ds, r)
        sums = g["table"].sum(axis=(3, 4), dtype=np.uint64)                       # every table holds its pairs, on either side
        assert np.array_equal(sums[:, :, 0], g["pairs"]) and np.array_equal(sums[:, :, 1], g["pairs"]), (what, G, ds, r)
    return True


@pytest.fixture(scope="module")
def ctx():
    p = _ctx(N_SIM)
    assert p.execute(phantom(N_SIM, 25, noise=4.0)), mp.last_error()
    yield p
    p.cleanup()


def _install(p, a, b):
    """Side a becomes the output of image 0, side b reference slot 2: both (NW, NW) uint8."""
    p.sim_set_reference(2, np.ascontiguousarray(b, dtype=np.uint8))
    return _set_out(p, np.pad(np.asarray(a, dtype=np.uint8), M)), np.asarray(b, dtype=np.uint8)


@pytest.fixture
def stepped(ctx):
    """The shared context with the random planes on both sides (other tests install their own)."""
    out, ref = _install(ctx, OUT, PLANE)
    return ctx, out, ref


@functools.lru_cache(maxsize=None)
def _wanted(G, ds):
    """The restatement of the random planes, once for the three workgroup counts: the regions alone, then the four of one call."""
    regions = shapes(ds)
    four = (FULL, (1, 3, 4, 1, ds[0], 1), regions[-2], (7, 5, 1, 3, 65, 65))       # the second one has no pair at any distance
    return regions, H.cooccurrence_statistics(OUT, PLANE, regions, G, ds), four, H.cooccurrence_statistics(OUT, PLANE, four, G, ds)


# 0: the launch's own number of workgroups, one a tile at these sizes; 3: the 25 tiles of the frame shared 9, 8, 8 and the smaller
# regions' tiles by fewer workgroups than tiles; 1: one workgroup walks every tile of a query. The tables do not depend on it.
@pytest.mark.parametrize("groups", [0, 3, 1])
@pytest.mark.parametrize("ds", DISTANCES)
@pytest.mark.parametrize("G", LEVELS)
def test_sim_cooccurrence_is_bit_identical(stepped, G, ds, groups, monkeypatch):
    p, out, ref = stepped
    if groups:
        monkeypatch.setenv("MUSICA_COOCCURRENCE_GROUPS", str(groups))   # read at every call
    regions, want, four, want_four = _wanted(G, ds)
    for k in range(len(regions)):                                       # each alone
        assert _same(p.sim_cooccurrence(_queries(regions[k:k + 1], 2), G, ds), want[k:k + 1], regions[k:k + 1], G, ds, ("alone", groups))
    assert len(four) == mp.COOCCURRENCE_MAX_QUERIES
    got = p.sim_cooccurrence(_queries(four, 2), G, ds)
    assert _same(got, want_four, four, G, ds, ("four", groups)) and not got[1]["pairs"].any() and not got[1]["table"].any()


def test_a_workgroup_takes_two_tiles():
    """The launcher gives a distance and side of a query of `tiles` tiles min(tiles, 256) workgroups (launchers.h: cooccurrence_groups,
    kCooccurrenceGroups); workgroup g takes the tiles g, g + 256, .. . A region of 1090 x 1030 is 18 x 17 = 306 tiles > 256: the
    workgroups 0 .. 49 take two tiles each, the others one; its last tiles are 2 and 6 wide. Random planes, d = 7 and 16."""
    n = 1120
    nw = n - 2 * M
    p = _ctx(n)
    rng = np.random.default_rng(15)
    assert p.execute(phantom(n, 5, noise=4.0)), mp.last_error()
    out = _set_out(p, np.pad(rng.integers(0, 256, (nw, nw), dtype=np.uint8), M))
    ref = rng.integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(3, ref)
    regions = [(7, 1, 3, 9, 1090, 1030)]
    assert -(-1090 // 64) * -(-1030 // 64) == 306 > 256
    assert _same(p.sim_cooccurrence(_queries(regions, 3), 32, (7, 16)), H.cooccurrence_statistics(out, ref, regions, 32, (7, 16)), regions, 32, (7, 16))
    p.cleanup()


def _counted(p, a, b, G, ds, region=FULL):
    out, ref = _install(p, a, b)
    got = p.sim_cooccurrence(_queries([region], 2), G, ds)
    assert _same(got, H.cooccurrence_statistics(out, ref, [region], G, ds), [region], G, ds)
    return got[0]["table"], got[0]["pairs"]


@pytest.mark.parametrize("G", LEVELS)
def test_contents_with_known_cells(ctx, G):
    p = ctx
    i, j = np.indices((NW, NW))   # i: the row, j: the column
    top = G - 1
    # vertical stripes of period 2 d: d columns of 0, d of 255. At distance d every horizontal and diagonal pair joins the two kinds,
    # every vertical pair two of one kind; at 2 d every pair joins two of one kind
    for d in (1, 3, 8):
        t, n = _counted(p, ((j // d) & 1) * 255, PLANE, G, (d, 2 * d))
        for direction in (0, 1, 3):
            assert t[0, direction, 0, 0, 0] == t[0, direction, 0, top, top] == 0
            assert int(t[0, direction, 0, 0, top]) + int(t[0, direction, 0, top, 0]) == int(n[0, direction])
        assert t[0, 2, 0, 0, top] == t[0, 2, 0, top, 0] == 0
        assert (t[1, :, 0, 0, top] == 0).all() and (t[1, :, 0, top, 0] == 0).all()
    # a one-pixel checkerboard: at distance 1 the horizontal and vertical pairs join the two kinds, the diagonal ones two of one kind
    t, n = _counted(p, ((i + j) & 1) * 255, PLANE, G, (1,))
    for direction, mixed in ((0, True), (1, False), (2, True), (3, False)):
        cells = int(t[0, direction, 0, 0, top]) + int(t[0, direction, 0, top, 0])
        assert cells == (int(n[0, direction]) if mixed else 0), direction
    # the level boundaries: the values k 2^shift - 1 and k 2^shift lie one level apart, and nothing else is on the plane
    step = 256 // G
    edges = np.array([v for k in range(1, G) for v in (k * step - 1, k * step)], dtype=np.uint8)
    a = edges[np.random.default_rng(31).integers(0, len(edges), (NW, NW))]
    b = edges[(i * 7 + j * 3) % len(edges)]
    t, n = _counted(p, a, b, G, (1, 16))
    assert t.any(axis=(0, 1, 2, 4)).all()      # every level, 0 and G - 1 included, is some pair's first


@pytest.mark.parametrize("groups", [0, 1])
def test_a_flat_plane_fills_one_counter(groups, monkeypatch):
    """Every pair of a flat plane against a flat slot falls into one counter of its table: 1024 x 1024 pixels in 256 tiles give the cell
    1024 * 1023 = 1047552 pairs at d = 1, and with MUSICA_COOCCURRENCE_GROUPS=1 all of them pass through ONE workgroup's counter, almost
    16 times what sixteen bits hold; with the default 256 workgroups a workgroup takes one tile of 64 * 63 .. 4096 pairs. The kernel has no
    packed counters and no flush rule (kernels_cooccurrence.hip, THE WIDTH RULE: u32 counters, a table below 2^28 pairs): this run is
    the proof that none of its counters is narrower than that, at G = 64 with one copy of a counter and at G = 8 with sixteen."""
    if groups:
        monkeypatch.setenv("MUSICA_COOCCURRENCE_GROUPS", str(groups))
    n = 1024 + 2 * M
    p = _ctx(n)
    assert p.execute(phantom(n, 5, noise=4.0)), mp.last_error()
    _set_out(p, np.full((n, n), 200, dtype=np.uint8))
    p.sim_set_reference(1, np.full((1024, 1024), 37, dtype=np.uint8))
    region = (0, 0, 0, 0, 1024, 1024)
    for G, ds in ((64, (1, 16)), (8, (1,))):
        got = p.sim_cooccurrence(_queries([region], 1), G, ds)[0]
        la, lb = 200 >> (8 - G.bit_length() + 1), 37 >> (8 - G.bit_length() + 1)
        assert int(got["pairs"][0, 0]) == 1024 * 1023 > 15 * 65535
        for k, d in enumerate(ds):
            want = [(1024 - d) * 1024, (1024 - d) ** 2, 1024 * (1024 - d), (1024 - d) ** 2]
            assert got["pairs"][k].tolist() == want
            assert got["table"][k, :, 0, la, la].tolist() == want and got["table"][k, :, 1, lb, lb].tolist() == want
        assert np.count_nonzero(got["table"]) == len(ds) * 4 * 2
    p.cleanup()


def test_marginals_are_the_joint_histograms(stepped):
    """The rows of the d = 1, 90 degree table run over the region's rows but the last: the table's row sums are the level histogram of
    that sub-rectangle, which musica_sim_joint counts on its own (the marginals of its 256 x 256 table, folded to G levels)."""
    p, out, ref = stepped
    for region in ((9, 3, 6, 11, 200, 136), FULL):
        ax, ay, bx, by, w, h = region
        joint = p.sim_joint(_queries([(ax, ay, bx, by, w, h - 1)], 2), tables=True)[0]["joint"].astype(np.int64)
        for G in LEVELS:
            t = p.sim_cooccurrence(_queries([region], 2), G, (1,))[0]["table"][0, 2].astype(np.int64)
            assert np.array_equal(t[0].sum(axis=1), joint.sum(axis=1).reshape(G, 256 // G).sum(axis=1))
            assert np.array_equal(t[1].sum(axis=1), joint.sum(axis=0).reshape(G, 256 // G).sum(axis=1))


def test_results_repeat_and_nothing_else_changes(stepped):
    p, out, ref = stepped
    graded, slot, inp = p.graded().copy(), p.sim_get_reference(2), p.input_pixels().copy()
    compared = p.sim_compare(_queries([FULL], 2))[0]
    for G in LEVELS:
        regions = [FULL, (9, 3, 6, 11, 200, 136), (1, 3, 4, 1, 1, 1)]
        first = p.sim_cooccurrence(_queries(regions, 2), G, (1, 2, 4, 8))
        p.sim_lattice(_queries([FULL], 2), 8, 2)                                     # something else in between
        p.sim_cooccurrence(_queries([FULL], 2), 64 if G != 64 else 8, (16,))         # other levels write the same buffers
        again = p.sim_cooccurrence(_queries(regions, 2), G, (1, 2, 4, 8))
        for a, b in zip(first, again):
            assert a["table"].tobytes() == b["table"].tobytes() and a["pairs"].tobytes() == b["pairs"].tobytes()
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(2), slot) and np.array_equal(p.input_pixels(), inp)
    again = p.sim_compare(_queries([FULL], 2))[0]
    assert all(again[k] == compared[k] for k in ("sq_diff_sum", "mse", "ssim"))


def test_every_word_is_written_and_nothing_behind(stepped):
    p, out, ref = stepped
    lib = mp.load_library()
    for G, ds in ((8, (1, 2, 4, 8)), (64, (16,))):
        regions = [(9, 3, 6, 11, 200, 136), (1, 3, 4, 1, 1, 1), (5, 7, 2, 1, 64, 64)]
        want = H.cooccurrence_statistics(out, ref, regions, G, ds)
        q = (mp.SimQuery * 3)(*[mp.SimQuery(*t) for t in _queries(regions, 2)])
        res = (mp.SimCooccurrenceResult * 3)()
        per = len(ds) * 8 * G * G
        guard = 0xA5A5A5A5
        tables = np.full(3 * per + 5, guard, dtype=np.uint32)
        dist = (mp.C.c_uint32 * len(ds))(*ds)
        assert lib.musica_sim_cooccurrence(p._h, G, len(ds), dist, 3, q, res, tables.ctypes.data_as(_U32P), 3 * per), mp.last_error()
        assert (tables[3 * per:] == guard).all()
        for k, (r, w) in enumerate(zip(res, want)):
            assert int(r.table_offset) == k * per
            pairs = [[int(r.pairs[i][j]) for j in range(4)] for i in range(mp.COOCCURRENCE_MAX_DISTANCES)]
            assert pairs[:len(ds)] == w["pairs"].tolist() and not np.any(pairs[len(ds):])
            assert np.array_equal(tables[k * per:(k + 1) * per].reshape(len(ds), 4, 2, G, G), w["table"])
        assert not tables[per:2 * per].any()      # the query without a pair: zeros, written


def test_two_images_of_a_batch():
    n = 150
    nw = n - 2 * M
    p = _ctx(n, batch=2)
    rng = np.random.default_rng(4)
    assert p.execute(np.stack([phantom(n, 1, noise=4.0), phantom(n, 2, noise=4.0)])), mp.last_error()
    outs = [_set_out(p, np.pad(rng.integers(0, 256, (nw, nw), dtype=np.uint8), M), k) for k in range(2)]
    ref = rng.integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(5, ref)
    region = (3, 1, 0, 2, 120, 127)
    got = p.sim_cooccurrence([(1, 5) + region, (0, 5) + region], 32, (2, 9))
    assert _same(got[:1], H.cooccurrence_statistics(outs[1], ref, [region], 32, (2, 9)), [region], 32, (2, 9))
    assert _same(got[1:], H.cooccurrence_statistics(outs[0], ref, [region], 32, (2, 9)), [region], 32, (2, 9))
    p.cleanup()


def test_refusals_leave_the_context_usable(stepped):
    p, out, ref = stepped
    lib = mp.load_library()
    q = (mp.SimQuery * 5)(*[mp.SimQuery(0, 2, 0, 0, 0, 0, 20, 20)] * 5)
    res = (mp.SimCooccurrenceResult * 5)()
    words = 5 * 4 * 8 * 64 * 64
    tables = np.zeros(words, dtype=np.uint32)
    tp = tables.ctypes.data_as(_U32P)
    one = (mp.C.c_uint32 * 1)(1)
    regions = shapes((1,))[:3]

    def usable():
        assert _same(p.sim_cooccurrence(_queries(regions, 2), 8, (1,)), H.cooccurrence_statistics(out, ref, regions, 8, (1,)), regions, 8, (1,))

    def refused(rc, text):
        assert rc == 0
        msg = mp.last_error()
        assert text in msg, msg
        usable()

    for bad in (0, 1, 4, 12, 24, 128, 1 << 20, 0xFFFFFFFF):
        refused(lib.musica_sim_cooccurrence(p._h, bad, 1, one, 1, q, res, tp, words), "levels")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, None, 1, q, res, tp, words), "distances is NULL")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 0, one, 1, q, res, tp, words), "distance_count")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 5, (mp.C.c_uint32 * 5)(1, 2, 3, 4, 5), 1, q, res, tp, words), "distance_count")
    for bad in ((0,), (17,), (1, 0xFFFFFFFF), (2, 2), (4, 3), (1, 2, 4, 3)):
        refused(lib.musica_sim_cooccurrence(p._h, 8, len(bad), (mp.C.c_uint32 * len(bad))(*bad), 1, q, res, tp, words), "distance ")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 0, q, res, tp, words), "count")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 5, q, res, tp, words), "count")
    refused(lib.musica_sim_cooccurrence(None, 8, 1, one, 1, q, res, tp, words), "NULL")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 1, None, res, tp, words), "NULL")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 1, q, None, tp, words), "NULL")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 1, q, res, None, words), "tables is NULL")
    refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 1, q, res, tp, 8 * 8 * 8 - 1), "table_words")
    refused(lib.musica_sim_cooccurrence(p._h, 64, 4, (mp.C.c_uint32 * 4)(1, 2, 4, 8), 4, q, res, tp, 4 * 4 * 8 * 64 * 64 - 1), "table_words")
    for bad, text in ((mp.SimQuery(0, 2, 0, 0, 0, 0, 0, 20), "side below 1"), (mp.SimQuery(0, 2, 0, 0, 0, 0, 20, 0), "side below 1"),
                      (mp.SimQuery(0, 5, 0, 0, 0, 0, 20, 20), "never written"), (mp.SimQuery(0, mp.SIM_SLOTS, 0, 0, 0, 0, 20, 20), "slot"),
                      (mp.SimQuery(1, 2, 0, 0, 0, 0, 20, 20), "image_index"), (mp.SimQuery(0, 2, NW - 19, 0, 0, 0, 20, 20), "leaves"),
                      (mp.SimQuery(0, 2, 0, 0, 0, NW - 19, 20, 20), "leaves")):
        refused(lib.musica_sim_cooccurrence(p._h, 8, 1, one, 1, (mp.SimQuery * 1)(bad), res, tp, words), text)
    assert not tables.any()                                # a refused call writes nothing
    for bad in (0, 4, 12, 128, -8, 8.5, "8", True, None):
        with pytest.raises(ValueError):
            p.sim_cooccurrence(_queries([FULL], 2), bad, (1,))
    for bad in ((), (0,), (17,), (2, 1), (1, 1), (1, 2, 3, 4, 5), (1.5,), "1", None, 3, (True,)):
        with pytest.raises(ValueError):
            p.sim_cooccurrence(_queries([FULL], 2), 8, bad)
    with pytest.raises(ValueError):
        p.sim_cooccurrence([], 8, (1,))
    with pytest.raises(ValueError):
        p.sim_cooccurrence(_queries([FULL] * 5, 2), 8, (1,))
    small = _ctx(2 * M)
    assert lib.musica_sim_cooccurrence(small._h, 8, 1, one, 1, q, res, tp, words) == 0 and "too small" in mp.last_error()
    small.cleanup()
    usable()


def _vendor(n, levels, seed):
    """A synthetic vendor image: the phantom of another seed processed here, as 16-bit stored values with noise in the low byte."""
    p = _ctx(n, levels)
    assert p.execute(phantom(n, seed + 100, noise=4.0)), mp.last_error()
    u = p.out_pixels()
    p.cleanup()
    low = np.random.default_rng(seed).integers(0, 256, size=u.shape, dtype=np.uint16)
    return ((255 - u.astype(np.uint16)) << 8) | low


def _study(n, levels, vendor, options, **runner_args):
    runner = H.Runner(n, levels, **runner_args)
    rows = H.run_study(phantom(n, 11, noise=4.0), runner, rng=np.random.default_rng(5), vendor=vendor, shutters=[], translations=H.scaled(H.TRANSLATIONS, n)[:1],
                       rotations=[], sigmas=[16.0], factors=[], **options)
    runner.close()
    return rows


@pytest.mark.parametrize("with_vendor, G, ds", [(True, 8, (1, 2, 4, 8)), (False, 32, (3, 16))])
def test_study_rows_agree_on_the_three_paths(with_vendor, G, ds):
    n, levels = 200, 4
    vendor = _vendor(n, levels, 7) if with_vendor else None
    parts = ("direct", "registered") + (("reference", "registered_reference") if with_vendor else ())
    keys = [part + "_texture" for part in parts]
    studies = {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = studies[name] = _study(n, levels, vendor, dict(texture=G, texture_distances=ds), **args)
        names = [r["alteration"] for r in rows]     # unaltered, the translations, a noise row
        assert names[0] == "unaltered" and names[-1].startswith("gn_") and len(names) >= 3, name
        for r in rows:                              # the texture keys stand behind all others; one for every comparison the row has
            mine = [k for k in r if k.endswith("_texture")]
            assert mine == [k for part, k in zip(parts, keys) if part in r] == list(r)[-len(mine):], (name, r["alteration"])
            for part, k in zip(parts, keys):
                if part in r and r[part] is None:
                    assert r[k] is None, (name, r["alteration"], part)
    # exact integers through one summary: equal on every path wherever the images are (the device's noise rows draw from another
    # stream than the host's)
    for h, d, a in zip(studies["host"], studies["metrics"], studies["alterations"]):
        for k in keys:
            if k in h:
                assert h[k] == d[k], (h["alteration"], k)
                if not h["alteration"].startswith("gn_"):
                    assert d[k] == a[k], (h["alteration"], k)
    first = studies["metrics"][0]["direct_texture"]      # the unaltered output against itself
    assert first["levels"] == G and first["distance_list"] == list(ds) and first["divergence"] == 0.0
    assert all(e["divergence"] == 0.0 and not any(e["difference"].values()) for e in first["distances"])
    assert studies["metrics"][-1]["direct_texture"]["divergence"] > 0.0   # noise changes the texture
