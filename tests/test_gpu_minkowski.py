"""The shape metric on the device: musica_sim_minkowski against metrics.minkowski_statistics, word for word, at the smallest shapes where
the kernel can go wrong: regions of one, two and three pixels a side, one-pixel rows and columns, regions below, at and just above the
64 x 64 tile, ragged last tiles and the 300 x 300 frame, at odd origins that differ between the sides; random bytes, all 0, all 255 (the
contention worst case), a 0 / 255 checkerboard, a plane that is 0 except in the columns and rows on either side of every tile seam (every
seam edge and corner is counted exactly once), planes constant over runs of 15, 16 and 17 pixels (the run merging and its boundaries)
and a processed phantom against a blurred copy; one and four queries a call, two images of a batch; workgroups that take several
tiles; that every word is written and nothing behind them; that results repeat; what the call must leave alone and its refusals; a
study's *_minkowski keys on its three paths. Everything compared is an integer: no tolerance anywhere."""
import functools

import numpy as np
import pytest
from scipy import ndimage

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import report
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

_U32P = mp.C.POINTER(mp.C.c_uint32)
M = mp.OUT_MARGIN
N_SIM = 320
NW = N_SIM - 2 * M
FULL = (0, 0, 0, 0, NW, NW)
PER = mp.MINKOWSKI_SIDES * mp.MINKOWSKI_KINDS * 256
OUT = np.random.default_rng(61).integers(0, 256, (NW, NW), dtype=np.uint8)
PLANE = np.random.default_rng(62).integers(0, 256, (NW, NW), dtype=np.uint8)
# (ax, ay, bx, by, w, h): odd ax and bx that differ, so that load_quant4's ragged ends differ between the sides
SHAPES = [(1, 3, 5, 1, 1, 1), (3, 1, 1, 2, 2, 2), (1, 5, 7, 3, 3, 3), (7, 3, 1, 4, 2, 40), (1, 2, 3, 1, 40, 1), (5, 1, 3, 2, 1, 40),
          (3, 3, 9, 1, 63, 63), (5, 7, 1, 1, 64, 64), (7, 5, 1, 3, 65, 65), (1, 1, 5, 2, 67, 67), (9, 3, 7, 11, 129, 70), (3, 9, 11, 5, 70, 129), FULL]
FOUR = (FULL, (1, 3, 5, 1, 3, 3), (9, 3, 7, 11, 129, 70), (7, 5, 1, 3, 65, 65))


def cells(w, h):
    """The number of cells of every kind of a w x h region."""
    return [w * h, h * (w + 1), (h + 1) * w, (h + 1) * (w + 1), h * (w - 1), (h - 1) * w, (h - 1) * (w - 1), 2 * w + 2 * h]


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


def _same(got, want, regions, what=None):
    assert len(got) == len(want) == len(regions)
    for g, w, r in zip(got, want, regions):
        assert set(g) == {"table", "pixels"}, what
        assert g["table"].dtype == np.uint32 and g["table"].shape == (3, 8, 256)
        assert g["pixels"] == w["pixels"] == r[4] * r[5], (what, r)
        assert np.array_equal(g["table"], w["table"]), (what, r, np.argwhere(g["table"] != w["table"])[:8].tolist())
        assert g["table"].sum(axis=2).tolist() == [cells(r[4], r[5])] * 3, (what, r)
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
def _wanted():
    """The restatement of the random planes, once for the three workgroup counts: the regions alone, then the four of one call."""
    return H.minkowski_statistics(OUT, PLANE, SHAPES), H.minkowski_statistics(OUT, PLANE, FOUR)


# 0: the launch's own number of workgroups, one a tile at these sizes; 3: the 25 tiles of the frame shared 9, 8, 8 and the smaller
# regions' tiles by fewer workgroups than tiles; 1: one workgroup walks every tile of a query. The tables do not depend on it.
def test_sim_minkowski_is_bit_identical_for_any_number_of_workgroups(stepped, monkeypatch):
    p, out, ref = stepped
    want, want_four = _wanted()
    seen = {}
    for groups in (0, 3, 1):
        if groups:
            monkeypatch.setenv("MUSICA_MINKOWSKI_GROUPS", str(groups))   # read at every call
        alone = [p.sim_minkowski(_queries(SHAPES[k:k + 1], 2))[0] for k in range(len(SHAPES))]
        assert _same(alone, want, SHAPES, ("alone", groups))
        assert len(FOUR) == mp.MINKOWSKI_MAX_QUERIES
        four = p.sim_minkowski(_queries(FOUR, 2))
        assert _same(four, want_four, FOUR, ("four", groups))
        seen[groups] = b"".join(r["table"].tobytes() for r in alone + four)
    assert seen[0] == seen[3] == seen[1]
    t = want[-1]["table"].astype(np.int64)
    assert np.array_equal(t[2, 0], np.bincount(np.minimum(OUT, PLANE).ravel(), minlength=256))


def _runs(length, seed):
    """Rows that are constant over runs of `length` pixels, from column 0 on: a lane's 16 pixels meet the runs' ends at every offset."""
    values = np.random.default_rng(seed).integers(0, 256, (NW, NW // length + 1), dtype=np.uint8)
    return np.repeat(values, length, axis=1)[:, :NW]


def _seams(level):
    """0 except in the columns and rows 63 and 64 of every tile of a region that starts at the origin."""
    i, j = np.indices((NW, NW))
    near = (j % 64 == 63) | (j % 64 == 0) & (j > 0) | (i % 64 == 63) | (i % 64 == 0) & (i > 0)
    return np.where(near, level, 0).astype(np.uint8)


def _checkerboard(phase):
    i, j = np.indices((NW, NW))
    return (((i + j + phase) & 1) * 255).astype(np.uint8)


SPECIAL = {
    "zeros": lambda: (np.zeros((NW, NW), np.uint8), np.zeros((NW, NW), np.uint8)),
    "all 255": lambda: (np.full((NW, NW), 255, np.uint8), np.full((NW, NW), 255, np.uint8)),
    "255 against random": lambda: (np.full((NW, NW), 255, np.uint8), OUT),
    "checkerboards": lambda: (_checkerboard(0), _checkerboard(1)),
    "seams": lambda: (_seams(200), (_seams(1).astype(np.uint16) * (1 + OUT % 251)).astype(np.uint8)),
    "runs of 15 and 16": lambda: (_runs(15, 1), _runs(16, 2)),
    "runs of 17 and 16": lambda: (_runs(17, 3), _runs(16, 4).T.copy()),
}


@pytest.mark.parametrize("kind", list(SPECIAL))
def test_special_planes(ctx, kind):
    a, b = SPECIAL[kind]()
    out, ref = _install(ctx, a, b)
    # the seams plane is laid out for regions that start at the origin: the frame, the tile sizes around 64 and the ragged ones from there too
    regions = SHAPES + [(0, 0, 0, 0, w, h) for w, h in ((63, 63), (64, 64), (65, 65), (67, 67), (129, 70), (70, 129))]
    want = H.minkowski_statistics(out, ref, regions)
    for k in range(0, len(regions), 4):
        assert _same(ctx.sim_minkowski(_queries(regions[k:k + 4], 2)), want[k:k + 4], regions[k:k + 4], kind)
    full = want[len(SHAPES) - 1]["table"]
    if kind == "all 255":
        assert full[:, :, 255].tolist() == [cells(NW, NW)] * 3
    if kind == "checkerboards":   # the two sides are never both bright: the minimum is empty; no two neighbours of a side are both bright
        assert full[2, :, 0].tolist() == cells(NW, NW) and full[0, 4:7, 0].tolist() == cells(NW, NW)[4:7]
        assert full[0, 1, 0] == NW and full[0, 2, 0] == NW and full[0, 3, 0] == 2   # of the closed cells only outline ones are dark: an edge a row or column, two corners


def test_a_processed_phantom_against_a_blurred_copy(ctx):
    p = ctx
    assert p.execute(phantom(N_SIM, 25, noise=4.0)), mp.last_error()
    out = p.out_pixels()
    blurred = ndimage.uniform_filter(out, 5)
    p.sim_set_reference(2, blurred)
    regions = [FULL, (9, 3, 7, 11, 200, 136), (1, 1, 5, 2, 67, 67)]
    got = p.sim_minkowski(_queries(regions, 2))
    assert _same(got, H.minkowski_statistics(out, blurred, regions), regions)
    row = H.minkowski_row(got[0])
    assert row["tv_a"] > row["tv_b"] > 0 and row["tv_gain"] > 1.0 and 0.0 < row["overlap"] < 1.0   # a blur shortens the iso-contours
    curves = H.minkowski_curves(got[0]["table"])
    assert int(curves[0, 0, 1:].sum()) == int(out.sum(dtype=np.int64)) and int(curves[1, 0, 1:].sum()) == int(blurred.sum(dtype=np.int64))
    tv = np.abs(np.diff(out.astype(np.int64), axis=0)).sum() + np.abs(np.diff(out.astype(np.int64), axis=1)).sum()
    assert int(curves[0, 1, 1:].sum()) == int(tv)


def test_results_repeat_and_nothing_else_changes(stepped):
    p, out, ref = stepped
    graded, slot, inp = p.graded().copy(), p.sim_get_reference(2), p.input_pixels().copy()
    compared = p.sim_compare(_queries([FULL], 2))[0]
    regions = [FULL, (9, 3, 7, 11, 129, 70), (1, 3, 5, 1, 1, 1)]
    first = p.sim_minkowski(_queries(regions, 2))
    p.sim_lattice(_queries([FULL], 2), 8, 2)             # something else in between
    p.sim_minkowski(_queries([(3, 3, 9, 1, 63, 63)], 2))   # another call writes the same buffers
    again = p.sim_minkowski(_queries(regions, 2))
    for a, b in zip(first, again):
        assert a["table"].tobytes() == b["table"].tobytes() and a["pixels"] == b["pixels"]
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(2), slot) and np.array_equal(p.input_pixels(), inp)
    assert np.array_equal(p.out_pixels(), out)
    after = p.sim_compare(_queries([FULL], 2))[0]
    assert all(after[k] == compared[k] for k in ("sq_diff_sum", "mse", "ssim"))
    assert np.array_equal(after["bins_a"], compared["bins_a"]) and np.array_equal(after["bins_b"], compared["bins_b"])
    assert np.array_equal(first[0]["table"][0, 0], compared["bins_a"]) and np.array_equal(first[0]["table"][1, 0], compared["bins_b"])


def test_every_word_is_written_and_nothing_behind(stepped):
    p, out, ref = stepped
    lib = mp.load_library()
    regions = [(9, 3, 7, 11, 129, 70), (1, 3, 5, 1, 1, 1), (5, 7, 1, 1, 64, 64)]
    want = H.minkowski_statistics(out, ref, regions)
    q = (mp.SimQuery * 3)(*[mp.SimQuery(*t) for t in _queries(regions, 2)])
    res = (mp.SimMinkowskiResult * 3)()
    guard = 0xA5A5A5A5
    for words in (3 * PER, 3 * PER + 5):
        tables = np.full(3 * PER + 5, guard, dtype=np.uint32)
        assert lib.musica_sim_minkowski(p._h, 3, q, res, tables.ctypes.data_as(_U32P), words), mp.last_error()
        assert (tables[3 * PER:] == guard).all()
        for k, (r, w) in enumerate(zip(res, want)):
            assert int(r.table_offset) == k * PER and int(r.pixels) == w["pixels"]
        assert np.array_equal(tables[:3 * PER].reshape(3, 3, 8, 256), np.stack([w["table"] for w in want]))   # the 1 x 1 region's empty kinds are written as 0


def test_two_images_of_a_batch():
    n = 150
    nw = n - 2 * M
    p = _ctx(n, batch=2)
    rng = np.random.default_rng(4)
    assert p.execute(np.stack([phantom(n, 1, noise=4.0), phantom(n, 2, noise=4.0)])), mp.last_error()
    outs = [_set_out(p, np.pad(rng.integers(0, 256, (nw, nw), dtype=np.uint8), M), k) for k in range(2)]
    ref = rng.integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(5, ref)
    region = (3, 1, 1, 2, 120, 127)
    got = p.sim_minkowski([(1, 5) + region, (0, 5) + region])
    assert _same(got[:1], H.minkowski_statistics(outs[1], ref, [region]), [region])
    assert _same(got[1:], H.minkowski_statistics(outs[0], ref, [region]), [region])
    p.cleanup()


def test_refusals_leave_the_context_usable(stepped):
    p, out, ref = stepped
    lib = mp.load_library()
    q = (mp.SimQuery * 5)(*[mp.SimQuery(0, 2, 0, 0, 0, 0, 20, 20)] * 5)
    res = (mp.SimMinkowskiResult * 5)()
    words = 5 * PER
    tables = np.zeros(words, dtype=np.uint32)
    tp = tables.ctypes.data_as(_U32P)
    regions = SHAPES[:4]

    def usable():
        assert _same(p.sim_minkowski(_queries(regions, 2)), H.minkowski_statistics(out, ref, regions), regions)

    def refused(rc, text):
        assert rc == 0
        msg = mp.last_error()
        assert text in msg, msg
        usable()

    refused(lib.musica_sim_minkowski(p._h, 0, q, res, tp, words), "count")             # what musica_sim_compare refuses comes first
    refused(lib.musica_sim_minkowski(p._h, 5, q, res, tp, words), "count")
    refused(lib.musica_sim_minkowski(p._h, 0, q, res, None, 0), "count")
    refused(lib.musica_sim_minkowski(p._h, 1, q, res, None, 0), "tables is NULL")      # then the tables,
    refused(lib.musica_sim_minkowski(p._h, 1, q, res, None, words), "tables is NULL")
    refused(lib.musica_sim_minkowski(p._h, 1, q, res, tp, PER - 1), "table_words")     # then their length
    refused(lib.musica_sim_minkowski(p._h, 4, q, res, tp, 4 * PER - 1), "table_words")
    refused(lib.musica_sim_minkowski(None, 1, q, res, tp, words), "NULL")
    refused(lib.musica_sim_minkowski(p._h, 1, None, res, tp, words), "NULL")
    refused(lib.musica_sim_minkowski(p._h, 1, q, None, tp, words), "NULL")
    for bad, text in ((mp.SimQuery(0, 2, 0, 0, 0, 0, 0, 20), "side below 1"), (mp.SimQuery(0, 2, 0, 0, 0, 0, 20, 0), "side below 1"),
                      (mp.SimQuery(0, 5, 0, 0, 0, 0, 20, 20), "never written"), (mp.SimQuery(0, mp.SIM_SLOTS, 0, 0, 0, 0, 20, 20), "slot"),
                      (mp.SimQuery(1, 2, 0, 0, 0, 0, 20, 20), "image_index"), (mp.SimQuery(0, 2, NW - 19, 0, 0, 0, 20, 20), "leaves"),
                      (mp.SimQuery(0, 2, 0, 0, 0, NW - 19, 20, 20), "leaves")):
        refused(lib.musica_sim_minkowski(p._h, 1, (mp.SimQuery * 1)(bad), res, None, 0), text)   # a region outside, in front of the tables
    assert not tables.any()                  # a refused call writes nothing
    with pytest.raises(ValueError):
        p.sim_minkowski([])
    with pytest.raises(ValueError):
        p.sim_minkowski(_queries([FULL] * 5, 2))
    small = _ctx(2 * M)
    assert lib.musica_sim_minkowski(small._h, 1, q, res, tp, words) == 0 and "too small" in mp.last_error()
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


def _equal(x, y):
    """Two *_minkowski values: the dicts without their curves, and the curves as arrays."""
    if x is None or y is None:
        return x is None and y is None
    plain = lambda d: {k: v for k, v in d.items() if k != "curves"}   # noqa: E731
    return plain(x) == plain(y) and ("curves" in x) == ("curves" in y) and ("curves" not in x or np.array_equal(x["curves"], y["curves"]))


@pytest.mark.parametrize("with_vendor, curves", [(True, False), (False, True)])
def test_study_rows_agree_on_the_three_paths(with_vendor, curves, tmp_path):
    n, levels = 200, 4
    vendor = _vendor(n, levels, 7) if with_vendor else None
    parts = ("direct", "registered") + (("reference", "registered_reference") if with_vendor else ())
    keys = [part + "_minkowski" for part in parts]
    studies, csvs = {}, {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = studies[name] = _study(n, levels, vendor, dict(minkowski=True, minkowski_curves=curves), **args)
        names = [r["alteration"] for r in rows]     # unaltered, the translations, a noise row
        assert names[0] == "unaltered" and names[-1].startswith("gn_") and len(names) >= 3, name
        for r in rows:                              # the keys stand behind all others; one for every comparison the row has
            mine = [k for k in r if k.endswith("_minkowski")]
            assert mine == [k for part, k in zip(parts, keys) if part in r] == list(r)[-len(mine):], (name, r["alteration"])
            for part, k in zip(parts, keys):
                if part in r and r[part] is None:
                    assert r[k] is None, (name, r["alteration"], part)
                if part in r and r[part] is not None:
                    assert ("curves" in r[k]) == curves
        kept = [r for r in rows if not r["alteration"].startswith("gn_")]
        report.write_studies_csvs([("a.raw", kept)], str(tmp_path / name))
        csvs[name] = (tmp_path / name / "minkowski_robustness.csv").read_bytes()
        if curves:
            written = report.write_minkowski_curves([("a.raw", kept)], str(tmp_path / name / "curves"))
            csvs[name] += open(written[0], "rb").read()
    # exact integers through one summary: equal on every path wherever the images are (the device's noise rows draw from another
    # stream than the host's)
    for h, d, a in zip(studies["host"], studies["metrics"], studies["alterations"]):
        for k in keys:
            if k in h:
                assert _equal(h[k], d[k]), (h["alteration"], k)
                if not h["alteration"].startswith("gn_"):
                    assert _equal(d[k], a[k]), (h["alteration"], k)
    assert csvs["host"] == csvs["metrics"] == csvs["alterations"]
    first = studies["metrics"][0]["direct_minkowski"]      # the unaltered output against itself
    assert first["overlap"] == 1.0 and first["overlap_min"] == 1.0 and first["tv_gain"] == 1.0 and first["area_l1"] == 0.0
    assert first["matched_perimeter_l1"] == 0.0 and first["matched_euler8_l1"] == 0.0 and first["pixels"] == (n - 2 * M) ** 2
