"""The contrast-detail pair on the device (kernels_details.hip): musica_alter_details against harness.insert_details and
musica_sim_details against harness.detail_statistics, bit for bit (discs across a tile corner, a tile with as many details as the
capacity argument allows, a disc over 3 x 3 tiles, boxes flush with the plane's corners and edges, tiles without a detail, the largest
list, the extreme contrasts, every store width, the study size), that they repeat and do not depend on the list's order, what they must
leave alone, their refusals, and the cd_ rows of a study on its three paths.

Nothing here asserts how visible a detail comes out: the numbers of a cd_ row are findings, not premises."""
import csv
import os

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

TOL = 1e-12   # what the similarity tests hold between the device metrics and numpy's
CONTRASTS = (512, -512, 1, -1, 100, -37)


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _full_range_u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    a[0, -1], a[-1, 0] = 65535, 0
    a[63, 63], a[63, 64], a[64, 63], a[64, 64] = 0, 65535, 1, 65535    # under the discs across the tile corner
    assert a.min() == 0 and a.max() == 65535
    return a


def _with_contrasts(details):
    return tuple((x, y, r, CONTRASTS[i % len(CONTRASTS)]) for i, (x, y, r) in enumerate(details))


def _corner_list(n):
    """For a side n >= 84: an r = 4 disc over the four tiles that meet at (63|64, 63|64), an r = 1 disc whose bounding square ends on
    the last column of tile 0 and one that starts on the first column of tile 1, r = 1 boxes flush with three corners of the plane and
    with its far edge; the rest of the plane has no detail."""
    return _with_contrasts([(63, 63, 4), (62, 20, 1), (65, 30, 1), (4, 4, 1), (n - 5, 4, 1), (4, n - 5, 1), (n - 5, n - 5, 1), (n - 5, 40, 1)])


def _packed_list(n):
    """r = 1 details at pitch 9 with centres 9, 18, ..: the discs that meet tile (1, 1) = [64, 128)^2 have their centres in [63, 128], eight
    to an axis, so that tile lists 64 details, what boxes of side 9 at pitch 9 allow (the capacity argument admits 67)."""
    centres = range(9, n - 4, 9)
    assert sum(1 for c in centres if 63 <= c <= 128) == 8
    return _with_contrasts([(x, y, 1) for y in centres for x in centres])


def _check(p, raw, details, image_index=0):
    p.alter_details(details, image_index)
    got = p.input_pixels()[image_index].copy()
    assert np.array_equal(got, H.insert_details(raw, details))
    return got


@pytest.mark.parametrize("n", [84, 88, 137])    # two tiles a side, the second ragged. 84 % 8 = 4: 4-byte words; 88: rows of whole 16-byte words, a chunk ends at the plane's edge; 137: odd, single pixels
def test_alter_details_is_bit_identical(n):
    raw = _full_range_u16(n, n)
    p = _ctx(n)
    p.alter_set_source(raw)
    lists = [_corner_list(n), ((63, 63, 1, 512),), ((64, 64, 2, -512),)]
    if n == 137:
        lists.append(_packed_list(n))
    for details in lists:
        got = _check(p, raw, details)
        p.alter_none()
        p.alter_details(details[::-1])                                            # a reversed list gives identical bytes
        assert np.array_equal(p.input_pixels()[0], got)
    for c in CONTRASTS:                                                           # each contrast over the four tiles' corner
        _check(p, raw, ((63, 63, 4, c), (n - 7, 20, 2, -c)))
    p.cleanup()


def test_alter_details_where_rows_are_whole_dwords_only():
    n = 90                                                                        # 90 % 8 = 2: the 4-byte words
    raw = _full_range_u16(n, 3)
    p = _ctx(n)
    p.alter_set_source(raw)
    _check(p, raw, _corner_list(n))
    p.cleanup()


def test_alter_details_over_three_by_three_tiles():
    n = 400
    raw = _full_range_u16(n, 4)
    p = _ctx(n)
    p.alter_set_source(raw)
    details = ((200, 200, 64, 512), (30, 30, 1, -512), (395, 395, 1, 1), (34, 360, 16, -1))   # the r = 64 disc spans columns and rows 136 .. 264
    got = _check(p, raw, details)
    assert int((got != raw).sum()) > 12000                                        # the large disc was written (12853 pixels, less those that stay)
    _check(p, raw, ((130, 130, 64, -512),))                                       # its box flush with the plane's corner
    _check(p, raw, ((n - 131, n - 131, 64, 100),))                                # ... and with its far corner
    p.cleanup()


def test_alter_details_with_the_largest_list():
    n = 520
    raw = _full_range_u16(n, 5)
    p = _ctx(n)
    p.alter_set_source(raw)
    details = _with_contrasts([(8 + 16 * j, 8 + 16 * i, 1) for i in range(32) for j in range(32)])
    assert len(details) == mp.DETAIL_MAX
    got = _check(p, raw, details)
    p.alter_details(details[::-1])
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
    for details in (_corner_list(n), H.detail_grid(n, -512), _packed_list(n)):
        p.alter_details(details, image_index=1)
        got = p.input_pixels()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2])
        assert np.array_equal(got[1], H.insert_details(raw, details))
    p.cleanup()


def test_alter_details_is_bit_identical_at_the_study_size():
    n = 3072
    raw = _full_range_u16(n, 7)
    p = _ctx(n)
    p.alter_set_source(raw)
    details = H.detail_grid(n, 128)
    assert len(details) == 324
    _check(p, raw, details)
    p.cleanup()


# ---- the measurement -------------------------------------------------------------------------------------------------------------------
N_SIM = 320
NW_SIM = N_SIM - 2 * mp.OUT_MARGIN
# an r = 64 box flush with the top-left corner of the 300-pixel output plane, r = 1 top-right, r = 2 bottom-left, r = 7 bottom-right
CORNERS = ((130, 130, 64, 1), (NW_SIM - 5, 4, 1, 1), (6, NW_SIM - 7, 2, 1), (NW_SIM - 17, NW_SIM - 17, 7, 1))
MANY = tuple((4 + 9 * j, 4 + 9 * i, 1, 1) for i in range(32) for j in range(32))


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


@pytest.mark.parametrize("name", ["random", "white"])
def test_sim_details_is_bit_identical(stepped, name):
    p, out = stepped
    plane = _planes()[name]
    p.sim_set_reference(2, plane)
    assert len(MANY) == mp.DETAIL_MAX
    for details in (CORNERS, CORNERS[::-1], CORNERS[:1], CORNERS[3:], ((150, 150, 64, 1),), MANY):
        got = p.sim_details(details, 2)
        assert got == H.detail_statistics(out, plane, details), (name, len(details))
        assert got == p.sim_details(details, 2)                                   # called twice: bit-equal
        for (x, y, r, _), s in zip(details[:8], got):                             # box_ssd is the compare call's integer over the same region
            ro = 2 * r + 2
            res = p.sim_compare([(0, 2, x - ro, y - ro, x - ro, y - ro, 4 * r + 5, 4 * r + 5)])[0]
            assert s["box_ssd"] == res["sq_diff_sum"] and s["box_pixels"] == res["pixels"]
    assert all(type(v) is int for v in got[0]["disc"].values())


def test_sim_details_against_an_all_zero_output():
    """A step on a constant image (min == max: nothing to normalise by): whatever it leaves in the output, the sums are the
    restatement's; where that is all 0, against the all-255 slot every partial sum of side b is at its largest."""
    p = _ctx(N_SIM)
    assert p.execute(np.full((N_SIM, N_SIM), 30000, np.uint16)), mp.last_error()
    out = p.out_pixels()
    white = np.full((NW_SIM, NW_SIM), 255, np.uint8)
    p.sim_set_reference(0, white)
    got = p.sim_details(CORNERS, 0)
    assert got == H.detail_statistics(out, white, CORNERS)
    if not out.any():
        assert got[0]["box_ssd"] == 65025 * 68121 and got[0]["ring"]["sum_bb"] == 65025 * 39408 and got[0]["disc"]["sum_ab"] == 0
    p.sim_capture(1)                                                              # the output against itself
    for s in p.sim_details(CORNERS, 1):
        assert s["box_ssd"] == 0
        for zone in ("disc", "ring"):
            assert s[zone]["sum_a"] == s[zone]["sum_b"] and s[zone]["sum_aa"] == s[zone]["sum_ab"] == s[zone]["sum_bb"]
    p.cleanup()


def test_sim_details_reads_the_named_image():
    n = 137
    nw = n - 2 * mp.OUT_MARGIN
    p = _ctx(n, batch=3)
    assert p.execute(np.stack([phantom(n, 30 + k, noise=4.0) for k in range(3)])), mp.last_error()
    plane = np.random.default_rng(1).integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(5, plane)
    details = ((42, 42, 20, 1), (4, nw - 5, 1, 1), (nw - 5, 4, 1, 1))             # an odd plane side, an r = 20 box flush with the top-left corner
    for k in range(3):
        assert p.sim_details(details, 5, image_index=k) == H.detail_statistics(p.out_pixels(k), plane, details), k
    p.cleanup()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _array(details):
    return (mp.Detail * len(details))(*[mp.Detail(*d) for d in details])


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
    res = (mp.SimDetailResult * mp.DETAIL_MAX)()
    ok = ((40, 40, 2, 8), (100, 40, 7, -8))

    def refused(rc, words):
        assert rc == 0
        msg = mp.last_error()
        assert words in msg, msg

    def both(details, words, plane=None, count=None):
        """The list is refused by both entry points (for the measurement in the output plane's coordinates when `plane` is its side)."""
        arr, count = _array(details), len(details) if count is None else count
        if plane in (None, n):
            refused(lib.musica_alter_details(p._h, 0, count, arr), words)
        if plane in (None, nw):
            refused(lib.musica_sim_details(p._h, 0, 0, count, arr, res), words)

    both(ok, "count", count=0)
    both(ok, "count", count=mp.DETAIL_MAX + 1)
    for r in (0, 65, 1 << 20):
        both(((130, 130, r, 8),), "radius")
    for c in (0, 513, -513):
        refused(lib.musica_alter_details(p._h, 0, 1, _array(((40, 40, 1, c),))), "contrast")
    assert lib.musica_sim_details(p._h, 0, 0, 1, _array(((40, 40, 1, 0),)), res) == 1    # the measurement does not look at it
    for d in ((3, 40, 1, 8), (40, 3, 1, 8), (-5, 40, 1, 8), (40, -5, 1, 8)):      # a box one pixel (or more) outside on the near sides
        both((d,), "leaves")
    for side in (n, nw):                                                          # ... and on the far sides of each plane
        both(((side - 4, 40, 1, 8),), "leaves", plane=side)
        both(((40, side - 4, 1, 8),), "leaves", plane=side)
    assert lib.musica_sim_details(p._h, 0, 0, 1, _array(((nw - 5, nw - 5, 1, 8),)), res) == 1   # flush is inside
    both(((40, 40, 1, 8), (48, 40, 1, 8)), "disjoint")                            # two boxes touching
    both(((40, 40, 1, 8), (48, 48, 1, 8)), "disjoint")
    both(((40, 40, 2, 8), (50, 44, 1, 8)), "disjoint")
    both(((40, 40, 1, 8), (100, 100, 1, 8), (40, 40, 1, 8)), "disjoint")          # the same detail twice
    refused(lib.musica_alter_details(None, 0, 2, _array(ok)), "NULL")
    refused(lib.musica_alter_details(p._h, 0, 2, None), "NULL")
    refused(lib.musica_sim_details(None, 0, 0, 2, _array(ok), res), "NULL")
    refused(lib.musica_sim_details(p._h, 0, 0, 2, None, res), "NULL")
    refused(lib.musica_sim_details(p._h, 0, 0, 2, _array(ok), None), "NULL")
    refused(lib.musica_alter_details(p._h, 1, 2, _array(ok)), "image_index")      # image_index == batch
    refused(lib.musica_alter_details(p._h, 1, 1, _array(((130, 130, 0, 8),))), "radius")   # a bad list AND a bad index: every alteration names its own arguments first
    refused(lib.musica_sim_details(p._h, 1, 0, 2, _array(ok), res), "image_index")
    refused(lib.musica_sim_details(p._h, 0, 5, 2, _array(ok), res), "never written")
    refused(lib.musica_sim_details(p._h, 0, mp.SIM_SLOTS, 2, _array(ok), res), "slot")
    for bad in (((40, 40, 0, 8),), ((40, 40, 1, 8), (48, 40, 1, 8)), ((3, 40, 1, 8),), ()):   # the binding refuses before the library
        with pytest.raises(ValueError):
            p.alter_details(bad)
        with pytest.raises(ValueError):
            p.sim_details(bad, 0)
    with pytest.raises(ValueError):
        p.alter_details(((40, 40, 1, 0),))
    fresh = _ctx(n, levels)
    refused(lib.musica_alter_details(fresh._h, 0, 2, _array(ok)), "no source")
    refused(lib.musica_sim_details(fresh._h, 0, 0, 2, _array(ok), res), "never written")
    small = _ctx(2 * mp.OUT_MARGIN)
    refused(lib.musica_sim_details(small._h, 0, 0, 2, _array(ok), res), "margin")
    small.cleanup()
    # nothing was touched by the refused calls (nor by the measurements that ran): no image, no result, no slot; slot 1 is unwritten
    assert np.array_equal(p.input_pixels(), inp) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    with pytest.raises(RuntimeError):
        p.sim_get_reference(1)
    # a successful insertion changes neither the last step's results nor a slot ...
    p.alter_details(ok)
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    assert p.sim_details(H.output_details(((60, 60, 2, 8),)), 0)[0]["box_ssd"] == 0   # the output is still the captured one
    # ... and the step on the resident buffer processes what the insertion wrote
    assert p.execute_device()
    p.sync()
    assert fresh.execute(H.insert_details(raw, ok))
    assert np.array_equal(p.graded(), fresh.graded())
    assert np.array_equal(p.input_pixels()[0], H.insert_details(raw, ok))
    assert p.sim_details(H.output_details(ok), 0) == H.detail_statistics(fresh.out_pixels(), slot0, H.output_details(ok))
    p.cleanup()
    fresh.cleanup()


# ---- the study -------------------------------------------------------------------------------------------------------------------------
def _grids(n):
    return dict(shutters=H.scaled(H.SHUTTERS, n)[:1], translations=H.scaled(H.TRANSLATIONS, n)[:1], rotations=[9], sigmas=[16.0], factors=[0.05])


def _study(n, details, **runner_args):
    runner = H.Runner(n, 0, **runner_args)
    rows = H.run_study(phantom(n, 11, noise=4.0), runner, rng=np.random.default_rng(5), scatters=[(3, 1, 2)], details=details,
                       detail_tables=details is not None, **_grids(n))
    runner.close()
    return rows


def test_study_rows_agree_on_the_three_paths():
    n = 201
    grids = H.DETAILS(n)
    studies = {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = _study(n, grids, **args)
        plain = _study(n, None, **args)
        assert [r["alteration"] for r in rows[len(plain):]] == ["cd_8", "cd_16", "cd_32", "cd_64", "cd_128"], name
        # the rows before them are the rows of the study without details, but for the key
        assert all(r["details"] is None for r in rows[:len(plain)]), name
        assert [{k: v for k, v in r.items() if k != "details"} for r in rows[:len(plain)]] == plain, name
        assert all("details" not in r for r in plain), name
        studies[name] = rows[len(plain):]
        for r in studies[name]:
            assert set(r) == {"alteration", "mean_cnr", "direct", "registered", "details"} and r["registered"] is None, (name, r["alteration"])
            d = r["details"]
            assert list(d["radii"]) == [1, 2, 4, 8] and all(g["count"] == 4 for g in d["radii"].values()) and len(d["per_detail"]) == 16
    assert studies["alterations"] == studies["metrics"]   # every number of every row, exactly
    for h, d in zip(studies["host"], studies["metrics"]):
        assert h["alteration"] == d["alteration"] and h["mean_cnr"] == d["mean_cnr"]
        assert h["details"] == d["details"], h["alteration"]                      # exact integers, one summary: equal to the last bit
        for k in mp.SIM_METRICS:
            assert abs(h["direct"][k] - d["direct"][k]) <= TOL, (h["alteration"], k, h["direct"][k], d["direct"][k])


def test_cli_details_writes_the_rows(tmp_path):
    out = str(tmp_path / "out")
    assert H.main(["--device-alterations", "--details", "--size", "512", "--levels", "5", "--out", out]) == 0
    names = ["cd_%d" % c for c in H.DETAIL_CONTRASTS]
    direct = list(csv.reader(open(os.path.join(out, "direct_robustness.csv"))))
    reg = list(csv.reader(open(os.path.join(out, "reg_based_robustness.csv"))))
    assert [r[1] for r in direct[-5:]] == names and not any(r[1].startswith("cd_") for r in reg)
    assert len(direct) == 1 + 30 + 5
    lines = list(csv.reader(open(os.path.join(out, "contrast_detail.csv"))))
    radii = sorted(set(d[2] for d in H.detail_grid(512, 8)))
    assert lines[0] == H.DETAIL_CSV_HEADER and [(l[1], int(l[2])) for l in lines[1:]] == [(name, r) for name in names for r in radii]
    assert all(int(l[3]) == len(H.detail_grid(512, 8)) // len(radii) for l in lines[1:])
    plain = str(tmp_path / "plain")
    assert H.main(["--device-alterations", "--size", "512", "--levels", "5", "--out", plain]) == 0
    assert not os.path.exists(os.path.join(plain, "contrast_detail.csv"))
    assert open(os.path.join(plain, "direct_robustness.csv")).read() == "".join(open(os.path.join(out, "direct_robustness.csv")).readlines()[:31])
