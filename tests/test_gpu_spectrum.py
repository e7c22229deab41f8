"""The spectrum metric on the device: musica_sim_spectrum against metrics.spectrum_statistics, word for word, at every tile side; regions
of one tile in a block that is otherwise empty, with remainders, with ragged last blocks in both axes, at odd unequal origins on the two
sides; one and four queries a call, one of them without a tile; workgroups that take several blocks; contents that put the energy in
known coefficients; the Parseval identity against the device's own compare; that results repeat; what the call must leave alone and its
refusals; a study's *_spectrum keys on its three paths. Everything compared is an integer: no tolerance anywhere."""
import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

_I64P = mp.C.POINTER(mp.C.c_int64)
M = mp.OUT_MARGIN
N_SIM = 320
NW = N_SIM - 2 * M
FULL = (0, 0, 0, 0, NW, NW)
TILES = (8, 16, 32, 64)
# (ax, ay, bx, by, w, h), each the smallest at which one thing can break. The origins are odd and differ between the sides wherever the
# frame leaves room, so that no load is 4-byte aligned.
SHAPES = {
    8: [(1, 3, 4, 1, 8, 8),            # one tile in a block that is otherwise empty
        (3, 1, 1, 2, 9, 15),           # the remainder is ignored: one tile
        (5, 7, 2, 1, 64, 64),          # a whole block
        (7, 5, 0, 3, 7, 290)],         # no tile
    # 200 x 136 is cut to 192 x 128 at both sides: 3 x 2 whole blocks behind a remainder. 216 x 152 is cut to 13 x 9 tiles of 16,
    # 208 x 144, and 232 x 168 to 7 x 5 tiles of 32, 224 x 160: the last block of either axis holds one tile's width or height
    16: [(5, 7, 2, 1, 64, 64), (9, 3, 6, 11, 200, 136), (9, 3, 6, 11, 216, 152)],
    32: [(5, 7, 2, 1, 64, 64), (9, 3, 6, 11, 200, 136), (9, 3, 6, 11, 232, 168)],
    64: [(5, 7, 2, 1, 64, 64), (11, 9, 1, 3, 130, 70), (9, 3, 6, 11, 200, 136)],   # 130 x 70: 2 x 1 tiles and remainders; 200 x 136: 3 x 2
}
# The full frame of 300 is cut to 296 (T = 8) and 288 (T = 16, 32): a last block 40 and 32 wide; to 256 at T = 64.
PLANE = np.random.default_rng(19).integers(0, 256, (NW, NW), dtype=np.uint8)


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


def _same(got, want, regions, T, what=None):
    assert len(got) == len(want) == len(regions)
    for g, w, r in zip(got, want, regions):
        assert set(g) == {"table", "tiles"}, what
        assert g["table"].dtype == np.int64 and g["table"].shape == (T, T, 3)
        assert np.array_equal(g["table"], w["table"]), (what, T, r)
        assert type(g["tiles"]) is int and g["tiles"] == w["tiles"] == (r[4] // T) * (r[5] // T), (what, T, r)
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


OUT = np.random.default_rng(18).integers(0, 256, (NW, NW), dtype=np.uint8)


@pytest.fixture
def stepped(ctx):
    """The shared context with the random planes on both sides (other tests install their own)."""
    out, ref = _install(ctx, OUT, PLANE)
    return ctx, out, ref


# 0: the launch's own number of workgroups, one a block at these sizes; 3: the 25 blocks of the frame shared 9, 8, 8 and the smaller
# regions' blocks by fewer workgroups than blocks; 1: one workgroup walks every block of a query. The tables do not depend on it.
@pytest.mark.parametrize("groups", [0, 3, 1])
@pytest.mark.parametrize("T", TILES)
def test_sim_spectrum_is_bit_identical(stepped, T, groups, monkeypatch):
    p, out, ref = stepped
    if groups:
        monkeypatch.setenv("MUSICA_SPECTRUM_GROUPS", str(groups))   # read at every call
    regions = SHAPES[T] + [FULL]
    want = H.spectrum_statistics(out, ref, regions, T)
    for k in range(len(regions)):                                     # each alone
        assert _same(p.sim_spectrum(_queries(regions[k:k + 1], 2), T), want[k:k + 1], regions[k:k + 1], T, ("alone", groups))
    # four queries of different sizes in one call, one of them without a tile
    four = [FULL, (7, 5, 0, 3, T - 1, 290), SHAPES[T][-1], (1, 3, 4, 1, T, T)]
    assert len(four) == mp.SPECTRUM_MAX_QUERIES
    want = H.spectrum_statistics(out, ref, four, T)
    got = p.sim_spectrum(_queries(four, 2), T)
    assert _same(got, want, four, T, ("four", groups)) and got[1]["tiles"] == 0 and not got[1]["table"].any()
    # identity 1 on the device's own numbers: the table against musica_sim_compare's sq_diff_sum of the region cut to whole tiles
    tiled = NW // T * T
    compared = p.sim_compare(_queries([(0, 0, 0, 0, tiled, tiled)], 2))[0]
    t = got[0]["table"]
    assert int(t[..., 0].sum()) + int(t[..., 1].sum()) - 2 * int(t[..., 2].sum()) == T * T * compared["sq_diff_sum"]


def test_a_workgroup_takes_two_blocks():
    """The launcher gives a query of `blocks` 64 x 64 blocks min(blocks, 768) workgroups (launchers.h: spectrum_groups, kSpectrumGroups);
    workgroup g takes the blocks g, g + 768, .. . A region of 1800 x 1795 at T = 16 is cut to 112 x 112 tiles = 1792 x 1792 pixels =
    28 x 28 = 784 blocks > 768: the workgroups 0 .. 15 take two blocks each, the others one. The second query, at odd unequal origins,
    holds 111 x 111 tiles = 1776 x 1776 pixels: 28 x 28 blocks again, the last of each axis 48 wide. Random planes."""
    n = 1820
    nw = n - 2 * M
    p = _ctx(n)
    rng = np.random.default_rng(15)
    assert p.execute(phantom(n, 5, noise=4.0)), mp.last_error()
    out = _set_out(p, np.pad(rng.integers(0, 256, (nw, nw), dtype=np.uint8), M))
    ref = rng.integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(3, ref)
    regions = [(0, 0, 0, 0, nw, 1795), (7, 1, 3, 9, 1790, 1789)]
    assert (nw // 16 * 16 // 64) ** 2 == 784 > 768 and -(-(1790 // 16 * 16) // 64) == 28
    assert _same(p.sim_spectrum(_queries(regions, 3), 16), H.spectrum_statistics(out, ref, regions, 16), regions, 16)
    p.cleanup()


def _energy(p, a, b, T, region=FULL):
    out, ref = _install(p, a, b)
    got = p.sim_spectrum(_queries([region], 2), T)
    assert _same(got, H.spectrum_statistics(out, ref, [region], T), [region], T)
    return got[0]["table"], got[0]["tiles"]


@pytest.mark.parametrize("T", TILES)
def test_contents_with_known_coefficients(ctx, T):
    p = ctx
    i, j = np.indices((NW, NW))   # i: the row, j: the column
    tiles = (NW // T) ** 2
    dc = 255 * T * T
    # all 255 against all 0: the largest coefficient there is, (255 T^2)^2 a tile, 2^40 at T = 64; nothing anywhere else
    t, n = _energy(p, np.full((NW, NW), 255), np.zeros((NW, NW)), T)
    assert n == tiles and int(t[0, 0, 0]) == tiles * dc * dc and np.count_nonzero(t) == 1
    if T == 64:
        assert 2 ** 39 < dc * dc < 2 ** 40
    # a one-pixel checkerboard: besides DC, all energy in [T - 1][T - 1]
    t, _ = _energy(p, ((i + j) & 1) * 255, PLANE, T)
    assert np.count_nonzero(t[..., 0]) == 2 and int(t[T - 1, T - 1, 0]) == tiles * (dc // 2) ** 2 == int(t[0, 0, 0])
    # one-pixel stripes: columns that alternate are the highest COLUMN sequency at row sequency 0, and the other way round
    t, _ = _energy(p, (j & 1) * 255, PLANE, T)
    assert np.count_nonzero(t[..., 0]) == 2 and int(t[0, T - 1, 0]) == tiles * (dc // 2) ** 2 and int(t[T - 1, 0, 0]) == 0
    t, _ = _energy(p, (i & 1) * 255, PLANE, T)
    assert np.count_nonzero(t[..., 0]) == 2 and int(t[T - 1, 0, 0]) == tiles * (dc // 2) ** 2 and int(t[0, T - 1, 0]) == 0
    # a single set pixel at each corner of a tile, in four tiles: |A| = 255 at every coefficient, the signs show in sum A B alone;
    # against a flat side b (sum A B at DC only) and against a random one (every sign of every Walsh function counts)
    a = np.zeros((NW, NW), dtype=np.uint8)
    for (ty, tx), (y, x) in zip(((0, 0), (0, 1), (1, 0), (1, 1)), ((0, 0), (0, T - 1), (T - 1, 0), (T - 1, T - 1))):
        a[ty * T + y, tx * T + x] = 255
    region = (0, 0, 0, 0, 2 * T, 2 * T)
    t, n = _energy(p, a, np.full((NW, NW), 7), T, region)
    assert n == 4 and (t[..., 0] == 4 * 255 * 255).all() and int(t[0, 0, 2]) == 4 * 255 * 7 * T * T and np.count_nonzero(t[..., 2]) == 1
    t, _ = _energy(p, a, PLANE, T, region)
    assert (t[..., 0] == 4 * 255 * 255).all() and (t[..., 2] < 0).any() and (t[..., 2] > 0).any()


def test_results_repeat_and_nothing_else_changes(stepped):
    p, out, ref = stepped
    graded, slot, inp = p.graded().copy(), p.sim_get_reference(2), p.input_pixels().copy()
    for T in TILES:
        regions = [FULL, SHAPES[T][-1], (1, 3, 4, 1, T, T)]
        first = p.sim_spectrum(_queries(regions, 2), T)
        p.sim_lattice(_queries([FULL], 2), 8, 2)                     # something else in between
        p.sim_spectrum(_queries([FULL], 2), 64 if T != 64 else 8)    # another tile side writes the same buffers
        again = p.sim_spectrum(_queries(regions, 2), T)
        for a, b in zip(first, again):
            assert a["table"].tobytes() == b["table"].tobytes() and a["tiles"] == b["tiles"]
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(2), slot) and np.array_equal(p.input_pixels(), inp)


def test_every_word_is_written_and_nothing_behind(stepped):
    p, out, ref = stepped
    lib = mp.load_library()
    for T in (8, 64):
        regions = [SHAPES[T][-1], (7, 5, 0, 3, T - 1, 290), (5, 7, 2, 1, 64, 64)]
        want = H.spectrum_statistics(out, ref, regions, T)
        q = (mp.SimQuery * 3)(*[mp.SimQuery(*t) for t in _queries(regions, 2)])
        res = (mp.SimSpectrumResult * 3)()
        per = T * T * 3
        guard = -0x5A5A5A5A5A5A5A5B
        tables = np.full(3 * per + 5, guard, dtype=np.int64)
        assert lib.musica_sim_spectrum(p._h, T, 3, q, res, tables.ctypes.data_as(_I64P), 3 * per), mp.last_error()
        assert (tables[3 * per:] == guard).all()
        for k, (r, w, region) in enumerate(zip(res, want, regions)):
            assert int(r.table_offset) == k * per and int(r.tiles) == w["tiles"]
            assert np.array_equal(tables[k * per:(k + 1) * per].reshape(T, T, 3), w["table"])
        assert not tables[per:2 * per].any()      # the query without a tile: zeros, written


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
    got = p.sim_spectrum([(1, 5) + region, (0, 5) + region], 32)
    assert _same(got[:1], H.spectrum_statistics(outs[1], ref, [region], 32), [region], 32)
    assert _same(got[1:], H.spectrum_statistics(outs[0], ref, [region], 32), [region], 32)
    p.cleanup()


def test_refusals_leave_the_context_usable(stepped):
    p, out, ref = stepped
    lib = mp.load_library()
    q = (mp.SimQuery * 5)(*[mp.SimQuery(0, 2, 0, 0, 0, 0, 20, 20)] * 5)
    res = (mp.SimSpectrumResult * 5)()
    words = 5 * 64 * 64 * 3
    tables = np.zeros(words, dtype=np.int64)
    tp = tables.ctypes.data_as(_I64P)

    def refused(rc, text):
        assert rc == 0
        msg = mp.last_error()
        assert text in msg, msg

    for bad in (0, 1, 4, 12, 24, 48, 128, 1 << 20, 0xFFFFFFFF):
        refused(lib.musica_sim_spectrum(p._h, bad, 1, q, res, tp, words), "tile")
    refused(lib.musica_sim_spectrum(p._h, 8, 0, q, res, tp, words), "count")
    refused(lib.musica_sim_spectrum(p._h, 8, 5, q, res, tp, words), "count")
    refused(lib.musica_sim_spectrum(None, 8, 1, q, res, tp, words), "NULL")
    refused(lib.musica_sim_spectrum(p._h, 8, 1, None, res, tp, words), "NULL")
    refused(lib.musica_sim_spectrum(p._h, 8, 1, q, None, tp, words), "NULL")
    refused(lib.musica_sim_spectrum(p._h, 8, 1, q, res, None, words), "tables is NULL")
    refused(lib.musica_sim_spectrum(p._h, 8, 1, q, res, tp, 8 * 8 * 3 - 1), "table_words")
    refused(lib.musica_sim_spectrum(p._h, 64, 4, q, res, tp, 4 * 64 * 64 * 3 - 1), "table_words")
    for bad, text in ((mp.SimQuery(0, 2, 0, 0, 0, 0, 0, 20), "side below 1"), (mp.SimQuery(0, 2, 0, 0, 0, 0, 20, 0), "side below 1"),
                      (mp.SimQuery(0, 5, 0, 0, 0, 0, 20, 20), "never written"), (mp.SimQuery(0, mp.SIM_SLOTS, 0, 0, 0, 0, 20, 20), "slot"),
                      (mp.SimQuery(1, 2, 0, 0, 0, 0, 20, 20), "image_index"), (mp.SimQuery(0, 2, NW - 19, 0, 0, 0, 20, 20), "leaves"),
                      (mp.SimQuery(0, 2, 0, 0, 0, NW - 19, 20, 20), "leaves")):
        one = (mp.SimQuery * 1)(bad)
        refused(lib.musica_sim_spectrum(p._h, 8, 1, one, res, tp, words), text)
    assert not tables.any()                                # a refused call writes nothing
    for bad in (0, 4, 12, 128, -8, 8.5, "8", True, None):
        with pytest.raises(ValueError):
            p.sim_spectrum(_queries([FULL], 2), bad)
    with pytest.raises(ValueError):
        p.sim_spectrum([], 8)
    with pytest.raises(ValueError):
        p.sim_spectrum(_queries([FULL] * 5, 2), 8)
    small = _ctx(2 * M)
    refused(lib.musica_sim_spectrum(small._h, 8, 1, q, res, tp, words), "too small")
    small.cleanup()
    regions = SHAPES[8][:2]
    assert _same(p.sim_spectrum(_queries(regions, 2), 8), H.spectrum_statistics(out, ref, regions, 8), regions, 8)


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


@pytest.mark.parametrize("with_vendor, T", [(True, 8), (False, 32)])
def test_study_rows_agree_on_the_three_paths(with_vendor, T):
    n, levels = 200, 4
    vendor = _vendor(n, levels, 7) if with_vendor else None
    parts = ("direct", "registered") + (("reference", "registered_reference") if with_vendor else ())
    keys = [part + "_spectrum" for part in parts]
    studies = {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = studies[name] = _study(n, levels, vendor, dict(spectrum=T), **args)
        names = [r["alteration"] for r in rows]     # unaltered, the translations, a noise row
        assert names[0] == "unaltered" and names[-1].startswith("gn_") and len(names) >= 3, name
        for r in rows:                              # the spectrum keys stand behind all others; one for every comparison the row has
            mine = [k for k in r if k.endswith("_spectrum")]
            assert mine == [k for part, k in zip(parts, keys) if part in r] == list(r)[-len(mine):], (name, r["alteration"])
            for part, k in zip(parts, keys):
                if part in r and r[part] is None:
                    assert r[k] is None, (name, r["alteration"], part)
    # exact integers through one summary: equal on every path, tables included, wherever the images are (the device's noise rows draw
    # from another stream than the host's)
    for h, d, a in zip(studies["host"], studies["metrics"], studies["alterations"]):
        for k in keys:
            if k in h:
                assert h[k] == d[k], (h["alteration"], k)
                if not h["alteration"].startswith("gn_"):
                    assert d[k] == a[k], (h["alteration"], k)
    first = studies["metrics"][0]["direct_spectrum"]
    assert first["tiles"] == ((n - 2 * M) // T) ** 2 and first["ac_gain"] == 1.0 and first["dc"] == 0.0
