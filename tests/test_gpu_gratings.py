"""The grating pair on the device (kernels_gratings.hip): musica_alter_gratings against harness.insert_gratings and musica_sim_gratings
against harness.grating_statistics, bit for bit (a plate across a tile corner, a tile with nine plates, a plate over 9 x 9 tiles, plates
flush with the plane's corners, tiles without a plate, the largest list, the longest period, wave vectors in every octant and along both
axes with both signs, waves at +-512 and 0, every store width, outputs that are random, all 0 and all 255), that they repeat and do not
depend on the list's order, what they must leave alone, their refusals, and the grating_ rows of a study on its three paths.

Nothing here asserts what gain MUSICA gives a grating: the numbers of a grating_ row are findings, not premises."""
import csv
import os

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

TOL = 1e-12   # what the similarity tests hold between the device metrics and numpy's
# (ux, uy, T) that a half-side of 8 admits (T <= 8): both axes with both signs, the four diagonals, the shortest periods, odd periods
SMALL = ((1, 0, 2), (0, 1, 2), (-1, 0, 3), (0, -1, 5), (1, 1, 2), (1, -1, 4), (-1, 1, 3), (-1, -1, 7), (2, 1, 4), (1, 2, 5), (-4, 1, 8), (3, -4, 8), (0, 1, 8),
         (1, 0, 8))
# ... and that need a larger one: the eight octants at the largest |u|, the longest period
WIDE = ((8, 3, 16), (3, 8, 16), (-8, 3, 16), (-3, 8, 16), (8, -3, 16), (3, -8, 16), (-8, -3, 16), (-3, -8, 16), (1, 0, 64), (0, 1, 64), (-1, 0, 64), (0, -1, 64),
        (8, 7, 64), (-7, 8, 33), (1, 1, 64), (5, -8, 17))


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _wave(t, seed):
    """A wave table that is no cosine: random in -512 .. 512 with both limits, and a 0 where there is room."""
    w = np.random.default_rng(1000 * t + seed).integers(-512, 513, t)
    w[0], w[-1] = 512, -512
    if t > 2:
        w[1] = 0
    return tuple(int(v) for v in w)


def _kinds(places, kinds, shift=0):
    """The places (x, y, h) as gratings, the kinds (ux, uy, T) cycling."""
    return tuple((x, y, h) + kinds[(i + shift) % len(kinds)][:2] + (kinds[(i + shift) % len(kinds)][2], _wave(kinds[(i + shift) % len(kinds)][2], i + shift))
                 for i, (x, y, h) in enumerate(places))


def _wraps(g):
    """Whether the phase of a grating wraps inside its region along a row and from row to row: a step of +1 in x (in y) changes it by
    something other than ux (uy)."""
    k = H.grating_phases(g[3], g[4], g[5], g[2])
    return bool((np.diff(k, axis=1) != g[3]).any()), bool((np.diff(k, axis=0) != g[4]).any())


def _full_range_u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    a[0, -1], a[-1, 0] = 65535, 0
    a[63, 63], a[63, 64], a[64, 63], a[64, 64] = 0, 65535, 1, 65535    # under the plate across the tile corner
    a[62, 63], a[63, 62] = 65535, 1
    return a


def _corner_lists(n):
    """For a side n >= 84. An h = 8 plate centred on (63, 63), over the four tiles that meet there, of every SMALL kind; every other tile
    has no plate. And h = 8 plates flush with the four corners of the plane and, where there is room, with its top and left edges."""
    flush = [(16, 16, 8), (n - 17, 16, 8), (16, n - 17, 8), (n - 17, n - 17, 8)]
    if n >= 3 * 33:
        flush += [(n // 2, 16, 8), (16, n // 2, 8)]
    return [_kinds([(63, 63, 8)], SMALL, s) for s in range(len(SMALL))] + [_kinds(flush, SMALL), _kinds(flush, SMALL, 7)]


def _packed_list(n, shift=0):
    """h = 8 plates at pitch 33 from the plane's corner: tile (1, 1) = [64, 128)^2 meets nine of them."""
    starts = range(0, n - 32, 33)
    assert sum(1 for s in starts if s <= 127 and s + 32 >= 64) == 3
    return _kinds([(x + 16, y + 16, 8) for y in starts for x in starts], SMALL, shift)


def _check(p, raw, gratings, image_index=0):
    p.alter_gratings(gratings, image_index)
    got = p.input_pixels()[image_index].copy()
    assert np.array_equal(got, H.insert_gratings(raw, gratings))
    return got


def test_the_lists_wrap_the_phase_both_ways():
    """What the kernels carry instead of dividing: the phase along a chunk (the insertion) and along a strand with its turn at the
    region's side (the measurement). Every kind used here wraps along a row where ux != 0 and from row to row where uy != 0."""
    for ux, uy, t in SMALL + WIDE:
        along, across = _wraps((0, 0, max(8, t), ux, uy, t, None))
        assert along == (ux != 0) and across == (uy != 0), (ux, uy, t)
    assert {(np.sign(ux), np.sign(uy)) for ux, uy, _ in SMALL + WIDE} == {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - {(0, 0)}


@pytest.mark.parametrize("n", [84, 88, 137])    # two tiles a side, the second ragged. 84 % 8 = 4: 4-byte words; 88: rows of whole 16-byte words, a chunk ends at the plane's edge; 137: odd, single pixels
def test_alter_gratings_is_bit_identical(n):
    raw = _full_range_u16(n, n)
    p = _ctx(n)
    p.alter_set_source(raw)
    lists = _corner_lists(n)
    if n == 137:
        lists += [_packed_list(n), _packed_list(n, 3), _kinds([(68, 68, 34)], WIDE, 13), _kinds([(33, 33, 16), (100, 100, 16), (33, 100, 16)], WIDE)]
    saturated = kept = 0
    for gratings in lists:
        got = _check(p, raw, gratings)
        saturated += int(((got == 65535) & (raw < 65535)).sum())
        kept += int(((got != 0) | (raw == 0)).all())
        p.alter_none()
        p.alter_gratings(gratings[::-1])                                          # a reversed list gives identical bytes
        assert np.array_equal(p.input_pixels()[0], got)
    assert saturated > 0 and kept == len(lists)                                   # some pixel clipped at 65535; no non-zero pixel became 0
    zero = tuple(g[:6] + ((0,) * g[5],) for g in lists[-1])
    assert np.array_equal(_check(p, raw, zero), raw)                              # a wave of zeros copies
    p.cleanup()


def test_alter_gratings_where_rows_are_whole_dwords_only():
    n = 90                                                                        # 90 % 8 = 2: the 4-byte words
    raw = _full_range_u16(n, 3)
    p = _ctx(n)
    p.alter_set_source(raw)
    for gratings in _corner_lists(n):
        _check(p, raw, gratings)
    p.cleanup()


def test_alter_gratings_over_nine_by_nine_tiles():
    n = 600
    raw = _full_range_u16(n, 4)
    p = _ctx(n)
    p.alter_set_source(raw)
    got = _check(p, raw, ((256, 256, 128, 8, 7, 64, _wave(64, 1)), (560, 560, 8, 1, -1, 2, _wave(2, 2))))   # the 513-pixel plate flush with the plane's corner
    assert int((got != raw).sum()) > 200000
    _check(p, raw, ((n - 257, n - 257, 128, -3, 8, 16, _wave(16, 3)), (18, 560, 9, 0, -1, 9, _wave(9, 4))))  # ... and with its far corner
    p.cleanup()


def test_alter_gratings_with_the_largest_list():
    n = 540
    raw = _full_range_u16(n, 5)
    p = _ctx(n)
    p.alter_set_source(raw)
    gratings = _kinds([(16 + 33 * j, 16 + 33 * i, 8) for i in range(16) for j in range(16)], SMALL)
    assert len(gratings) == mp.GRATING_MAX
    got = _check(p, raw, gratings)
    p.alter_gratings(gratings[::-1])
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
    for gratings in (_corner_lists(n)[-2], H.grating_grid(n, -512), _packed_list(n)):
        p.alter_gratings(gratings, image_index=1)
        got = p.input_pixels()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2])
        assert np.array_equal(got[1], H.insert_gratings(raw, gratings))
    p.cleanup()


# ---- the measurement -------------------------------------------------------------------------------------------------------------------
N_SIM = 320
NW_SIM = N_SIM - 2 * mp.OUT_MARGIN
# plates flush with the four corners of the 300-pixel output plane: h = 8 top-left, h = 9 top-right, h = 31 bottom-left, h = 40 bottom-right
CORNERS = _kinds([(16, 16, 8), (NW_SIM - 19, 18, 9), (62, NW_SIM - 63, 31), (NW_SIM - 81, NW_SIM - 81, 40)], SMALL, 2)
LARGE = [_kinds([(148 + i % 3, 148 + i % 2, 74)], WIDE, i) for i in range(len(WIDE))]
MANY = _kinds([(16 + 33 * j, 16 + 33 * i, 8) for i in range(9) for j in range(9)], SMALL)
MIXED = _kinds([(34, 34, 17), (110, 40, 16), (200, 50, 20), (70, 150, 33), (220, 200, 32)], WIDE, 3)


def _set_out(p, values, image_index=0):
    """Makes the 8-bit output of an image `values` ((N, N) integers 0 .. 255; the margin is cropped): graded = (v + 0.5) / 255."""
    p.set_image(mp.IMG_GRADED, 0, ((np.asarray(values) + 0.5) / 255.0).astype(np.float32), image_index=image_index)
    m = mp.OUT_MARGIN
    out = p.out_pixels(image_index)
    assert np.array_equal(out, np.asarray(values)[m:-m, m:-m])
    return out


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for k in w:
            if k in mp.GRATING_SUMS:
                assert g[k].dtype == np.uint32 and np.array_equal(g[k], w[k]), k
            else:
                assert type(g[k]) is int and g[k] == w[k], k
    return True


def _outputs(n):
    rng = np.random.default_rng(8)
    random = rng.integers(0, 256, (n, n), dtype=np.uint8)
    random[mp.OUT_MARGIN, mp.OUT_MARGIN], random[-mp.OUT_MARGIN - 1, -mp.OUT_MARGIN - 1] = 0, 255
    return {"random": random, "white": np.full((n, n), 255, np.uint8), "zero": np.zeros((n, n), np.uint8)}


@pytest.fixture(scope="module")
def stepped():
    p = _ctx(N_SIM)
    assert p.execute(phantom(N_SIM, 25, noise=4.0)), mp.last_error()
    yield p
    p.cleanup()


@pytest.mark.parametrize("name", ["random", "white", "zero"])
def test_sim_gratings_is_bit_identical(stepped, name):
    p = stepped
    out = _set_out(p, _outputs(N_SIM)[name])
    plane = np.random.default_rng(9).integers(0, 256, (NW_SIM, NW_SIM), dtype=np.uint8)
    p.sim_set_reference(2, plane)
    for gratings in [CORNERS, CORNERS[::-1], CORNERS[:1], CORNERS[3:], MIXED, MANY] + LARGE:
        got = p.sim_gratings(gratings, 2)
        assert _same(got, H.grating_statistics(out, plane, gratings)), (name, len(gratings))
        for g, s in zip(gratings[:6], got):                                       # roi_ssd is the compare call's integer over the same region
            x, y, h = g[:3]
            res = p.sim_compare([(0, 2, x - h, y - h, x - h, y - h, 2 * h + 1, 2 * h + 1)])[0]
            assert s["roi_ssd"] == res["sq_diff_sum"] and s["roi_pixels"] == res["pixels"]
            side = 2 * h + 1
            assert int(s["n"].sum()) == s["roi_pixels"] and s["n"].min() > 0 and int(s["n"].max()) <= (side + 1) // 2 * side and s["T"] == g[5]
    assert _same(p.sim_gratings(MANY[::-1], 2), H.grating_statistics(out, plane, MANY)[::-1])
    p.sim_set_reference(3, np.full((NW_SIM, NW_SIM), 255, np.uint8))              # ... and against the all-255 slot: side b at its largest
    for gratings in (CORNERS, LARGE[0], LARGE[9]):
        assert _same(p.sim_gratings(gratings, 3), H.grating_statistics(out, np.full((NW_SIM, NW_SIM), 255, np.uint8), gratings))


def test_sim_gratings_returns_identical_bytes_twice(stepped):
    p = stepped
    _set_out(p, _outputs(N_SIM)["random"])
    p.sim_capture(4)
    lib = mp.load_library()
    gs = MIXED + _kinds([(280, 20, 8)], SMALL, 2)
    arr = (mp.Grating * len(gs))(*[mp.Grating(*g[:6]) for g in gs])
    words = 4 * sum(g[5] for g in gs)
    runs = []
    for _ in range(2):
        res, tables = (mp.SimGratingResult * len(gs))(), np.zeros(words, np.uint32)
        assert lib.musica_sim_gratings(p._h, 0, 4, len(gs), arr, res, tables.ctypes.data_as(mp._U32P), words) == 1, mp.last_error()
        runs.append((bytes(res), tables.tobytes()))
    assert runs[0] == runs[1]
    assert all(r.roi_ssd == 0 for r in res)                                       # the output against itself


def test_sim_gratings_at_the_u32_bound():
    """The largest region (S = 257) of an all-255 output folded into two bins: 129 * 257 = 33153 pixels in bin 0, sum_aa = 33153 * 255^2
    = 2155773825 > 2^31; and the longest period, T = 64, at the largest half-side, along both axes with both signs and in a steep
    direction."""
    n = 540
    nw = n - 2 * mp.OUT_MARGIN
    p = _ctx(n)
    assert p.execute(phantom(n, 26, noise=4.0)), mp.last_error()
    out = _set_out(p, np.full((n, n), 255, np.uint8))
    plane = np.random.default_rng(2).integers(0, 256, (nw, nw), dtype=np.uint8)
    p.sim_set_reference(1, plane)
    for ux, uy, t in ((0, 1, 2), (1, 0, 2), (1, 1, 2), (0, -1, 64), (-1, 0, 64), (1, 0, 64), (0, 1, 64), (8, -7, 64), (-1, 8, 64)):
        gratings = ((258, 260, 128, ux, uy, t, None),)
        got = p.sim_gratings(gratings, 1)
        assert _same(got, H.grating_statistics(out, plane, gratings)), (ux, uy, t)
        if t == 2 and 0 in (ux, uy):
            assert int(got[0]["n"][0]) == 33153 and int(got[0]["sum_aa"][0]) == 2155773825
    out = _set_out(p, np.random.default_rng(3).integers(0, 256, (n, n), dtype=np.uint8))
    for ux, uy, t in ((0, -1, 64), (1, 0, 64), (8, 7, 64), (-7, -8, 63)):
        gratings = ((258, 260, 128, ux, uy, t, None),)
        assert _same(p.sim_gratings(gratings, 1), H.grating_statistics(out, plane, gratings)), (ux, uy, t)
    p.cleanup()


def test_sim_gratings_reads_the_named_image_and_slot():
    n = 137
    nw = n - 2 * mp.OUT_MARGIN
    p = _ctx(n, batch=3)
    assert p.execute(np.stack([phantom(n, 30 + k, noise=4.0) for k in range(3)])), mp.last_error()
    planes = {5: np.random.default_rng(1).integers(0, 256, (nw, nw), dtype=np.uint8), 6: np.random.default_rng(2).integers(0, 256, (nw, nw), dtype=np.uint8)}
    for slot, plane in planes.items():
        p.sim_set_reference(slot, plane)
    gratings = _kinds([(nw - 17, 16, 8), (16, nw - 17, 8), (20, 20, 10), (nw - 19, nw - 19, 9)], SMALL, 5)   # an odd plane side, plates flush with its corners
    for k in range(3):
        for slot, plane in planes.items():
            assert _same(p.sim_gratings(gratings, slot, image_index=k), H.grating_statistics(p.out_pixels(k), plane, gratings)), (k, slot)
    p.cleanup()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _array(gratings):
    return (mp.Grating * len(gratings))(*[mp.Grating(*g[:6]) for g in gratings])


def _waves(gratings):
    w = np.array([v for g in gratings for v in g[6]], dtype=np.int16)
    return w, w.ctypes.data_as(mp.C.POINTER(mp.C.c_int16))


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
    words = 4 * mp.GRATING_MAX_PERIOD * 4
    res = (mp.SimGratingResult * mp.GRATING_MAX)()
    tables = np.full(words, 0xDEADBEEF, np.uint32)
    tp = tables.ctypes.data_as(mp._U32P)
    ok = ((60, 60, 8, 1, 0, 8, H.grating_wave(8, 8)), (150, 60, 16, 2, -3, 7, H.grating_wave(7, -8)))
    zeros = np.zeros(mp.GRATING_MAX * mp.GRATING_MAX_PERIOD, np.int16)
    zp = zeros.ctypes.data_as(mp.C.POINTER(mp.C.c_int16))

    def refused(rc, text):
        assert rc == 0
        msg = mp.last_error()
        assert text in msg, msg
        # ... and a good call goes through behind every refusal
        assert lib.musica_sim_gratings(p._h, 0, 0, 1, _array(ok[:1]), res, scratch.ctypes.data_as(mp._U32P), scratch.size) == 1, mp.last_error()
        assert res[0].bins == 8 and res[0].roi_ssd == 0 and res[0].roi_pixels == 289 and int(scratch[:8].sum()) == 289

    scratch = np.zeros(32, np.uint32)

    def both(gratings, text, plane=None, count=None):
        """The list is refused by both entry points (for the measurement in the output plane's coordinates when `plane` is its side)."""
        arr, count = _array(gratings), len(gratings) if count is None else count
        if plane in (None, n):
            refused(lib.musica_alter_gratings(p._h, 0, count, arr, zp, zeros.size), text)
        if plane in (None, nw):
            refused(lib.musica_sim_gratings(p._h, 0, 0, count, arr, res, tp, words), text)

    both(ok, "count", count=0)
    both(ok, "count", count=mp.GRATING_MAX + 1)
    for h in (0, 7, 129, 1 << 20):
        both(((130, 130, h, 1, 0, 8, None),), "half-side")
    for u in ((0, 0), (9, 1), (1, 9), (-9, 1), (1, -9), (2, 2), (4, 2), (0, 2), (-3, 0), (1 << 20, 1)):
        both(((130, 130, 32, u[0], u[1], 32, None),), "wave vector")
    for g in ((60, 60, 8, 1, 0, 1), (60, 60, 8, 1, 0, 0), (60, 60, 8, 1, 0, 9), (130, 130, 128, 1, 0, 65), (130, 130, 32, 8, 1, 15), (130, 130, 32, 1, -8, 15),
              (60, 60, 8, 1, 0, 1 << 31)):
        both((g + (None,),), "period")
    for g in ((15, 60, 8, 1, 0, 8, None), (60, 15, 8, 1, 0, 8, None), (-60, 60, 8, 1, 0, 8, None), (60, -60, 8, 1, 0, 8, None)):   # one pixel (or more) outside on the near sides
        both((g,), "leaves")
    for side in (n, nw):                                                          # ... and on the far sides of each plane
        both(((side - 16, 60, 8, 1, 0, 8, None),), "leaves", plane=side)
        both(((60, side - 16, 8, 1, 0, 8, None),), "leaves", plane=side)
    both(((60, 60, 8, 1, 0, 8, None), (92, 60, 8, 1, 0, 8, None)), "disjoint")    # two plates sharing a column
    both(((60, 60, 8, 1, 0, 8, None), (92, 92, 8, 1, 0, 8, None)), "disjoint")
    both(((60, 60, 8, 1, 0, 8, None), (108, 70, 16, 1, 0, 8, None)), "disjoint")
    both(ok + ok[:1], "disjoint")                                                 # the same grating twice
    w, wp = _waves(ok)
    refused(lib.musica_alter_gratings(None, 0, 2, _array(ok), wp, w.size), "NULL")
    refused(lib.musica_alter_gratings(p._h, 0, 2, None, wp, w.size), "NULL")
    refused(lib.musica_alter_gratings(p._h, 0, 2, _array(ok), None, w.size), "NULL")
    refused(lib.musica_alter_gratings(p._h, 0, 2, _array(ok), wp, w.size - 1), "wave_words")
    refused(lib.musica_alter_gratings(p._h, 0, 2, _array(ok), wp, 0), "wave_words")
    for at, v in ((0, 513), (14, -513), (7, 32767), (8, -32768)):
        bad = w.copy()
        bad[at] = v
        refused(lib.musica_alter_gratings(p._h, 0, 2, _array(ok), bad.ctypes.data_as(mp.C.POINTER(mp.C.c_int16)), bad.size), "wave entry")
    refused(lib.musica_sim_gratings(None, 0, 0, 2, _array(ok), res, tp, words), "NULL")
    refused(lib.musica_sim_gratings(p._h, 0, 0, 2, None, res, tp, words), "NULL")
    refused(lib.musica_sim_gratings(p._h, 0, 0, 2, _array(ok), None, tp, words), "NULL")
    refused(lib.musica_sim_gratings(p._h, 0, 0, 2, _array(ok), res, None, words), "NULL")
    need = 4 * (8 + 7)
    refused(lib.musica_sim_gratings(p._h, 0, 0, 2, _array(ok), res, tp, need - 1), "table_words")
    refused(lib.musica_sim_gratings(p._h, 0, 0, 2, _array(ok), res, tp, 0), "table_words")
    refused(lib.musica_alter_gratings(p._h, 1, 2, _array(ok), wp, w.size), "image_index")        # image_index == batch
    refused(lib.musica_alter_gratings(p._h, 1, 1, _array(((130, 130, 0, 1, 0, 8, None),)), zp, zeros.size), "half-side")   # a bad list AND a bad index: every alteration names its own arguments first
    refused(lib.musica_sim_gratings(p._h, 1, 0, 2, _array(ok), res, tp, words), "image_index")
    refused(lib.musica_sim_gratings(p._h, 0, 5, 2, _array(ok), res, tp, words), "never written")
    refused(lib.musica_sim_gratings(p._h, 0, mp.SIM_SLOTS, 2, _array(ok), res, tp, words), "slot")
    assert (tables == 0xDEADBEEF).all()                                           # no refused call wrote a word of the tables
    assert lib.musica_sim_gratings(p._h, 0, 0, 2, _array(ok), res, tp, need) == 1  # exactly enough room
    assert (tables[need:] == 0xDEADBEEF).all() and res[1].table_offset == 32 and res[1].bins == 7 and res[0].table_offset == 0
    for bad in (((60, 60, 7, 1, 0, 4, (0,) * 4),), ((60, 60, 8, 1, 0, 8, (0,) * 8), (92, 60, 8, 1, 0, 8, (0,) * 8)), ((15, 60, 8, 1, 0, 8, (0,) * 8),),
                ((60, 60, 8, 2, 2, 8, (0,) * 8),), ((60, 60, 8, 1, 0, 9, (0,) * 9),), ()):   # the binding refuses before the library
        with pytest.raises(ValueError):
            p.alter_gratings(bad)
        with pytest.raises(ValueError):
            p.sim_gratings(bad, 0)
    for wave in ((0,) * 7, (0,) * 9, (513,) + (0,) * 7, None):
        with pytest.raises(ValueError):
            p.alter_gratings(((60, 60, 8, 1, 0, 8, wave),))
    fresh = _ctx(n, levels)
    assert lib.musica_alter_gratings(fresh._h, 0, 2, _array(ok), wp, w.size) == 0 and "no source" in mp.last_error()
    assert lib.musica_sim_gratings(fresh._h, 0, 0, 2, _array(ok), res, tp, words) == 0 and "never written" in mp.last_error()
    small = _ctx(2 * mp.OUT_MARGIN)
    assert lib.musica_sim_gratings(small._h, 0, 0, 2, _array(ok), res, tp, words) == 0 and "margin" in mp.last_error()
    small.cleanup()
    # nothing was touched by the refused calls (nor by the measurements that ran): no image, no result, no slot; slot 1 is unwritten
    assert np.array_equal(p.input_pixels(), inp) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    with pytest.raises(RuntimeError):
        p.sim_get_reference(1)
    # a successful insertion changes neither the last step's results nor a slot ...
    p.alter_gratings(ok)
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    assert p.sim_gratings(H.output_gratings(ok[:1]), 0)[0]["roi_ssd"] == 0        # the output is still the captured one
    # ... and the step on the resident buffer processes what the insertion wrote
    assert p.execute_device()
    p.sync()
    assert fresh.execute(H.insert_gratings(raw, ok))
    assert np.array_equal(p.graded(), fresh.graded())
    assert np.array_equal(p.input_pixels()[0], H.insert_gratings(raw, ok))
    assert _same(p.sim_gratings(H.output_gratings(ok), 0), H.grating_statistics(fresh.out_pixels(), slot0, H.output_gratings(ok)))
    p.cleanup()
    fresh.cleanup()


# ---- the study -------------------------------------------------------------------------------------------------------------------------
def _grids(n):
    return dict(shutters=H.scaled(H.SHUTTERS, n)[:1], translations=H.scaled(H.TRANSLATIONS, n)[:1], rotations=[9], sigmas=[16.0], factors=[0.05])


def _study(n, gratings, **runner_args):
    runner = H.Runner(n, 0, **runner_args)
    rows = H.run_study(phantom(n, 11, noise=4.0), runner, rng=np.random.default_rng(5), scatters=[(3, 1, 2)], gratings=gratings,
                       grating_tables=gratings is not None, **_grids(n))
    runner.close()
    return rows


def test_study_rows_agree_on_the_three_paths():
    n = 201
    grids = H.GRATINGS(n)
    studies = {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = _study(n, grids, **args)
        plain = _study(n, None, **args)
        assert [r["alteration"] for r in rows[len(plain):]] == ["grating_8", "grating_16", "grating_32", "grating_64", "grating_128"], name
        # the rows before them are the rows of the study without gratings, but for the key
        assert all(r["gratings"] is None for r in rows[:len(plain)]), name
        assert [{k: v for k, v in r.items() if k != "gratings"} for r in rows[:len(plain)]] == plain, name
        assert all("gratings" not in r for r in plain), name
        studies[name] = rows[len(plain):]
        for r in studies[name]:
            assert set(r) == {"alteration", "mean_cnr", "direct", "registered", "gratings"} and r["registered"] is None, (name, r["alteration"])
            d = r["gratings"]
            assert list(d["directions"]) == ["1,0", "0,1", "1,1", "1,-1"] and list(d["periods"]) == [2, 3, 4] and d["all"]["gratings"] == 9
            assert len(d["per_grating"]) == 9 and all(len(g["folded"][side]) == g["T"] for g in d["per_grating"] for side in H.GRATING_SIDES)
    assert studies["alterations"] == studies["metrics"]   # every number of every row, exactly
    for h, d in zip(studies["host"], studies["metrics"]):
        assert h["alteration"] == d["alteration"] and h["mean_cnr"] == d["mean_cnr"]
        assert h["gratings"] == d["gratings"], h["alteration"]                    # exact integers, one summary: equal to the last bit
        for k in mp.SIM_METRICS:
            assert abs(h["direct"][k] - d["direct"][k]) <= TOL, (h["alteration"], k, h["direct"][k], d["direct"][k])


def test_cli_gratings_writes_the_rows(tmp_path):
    out = str(tmp_path / "out")
    assert H.main(["--device-alterations", "--gratings", "--size", "512", "--levels", "5", "--out", out]) == 0
    names = ["grating_%d" % c for c in H.GRATING_CONTRASTS]
    direct = list(csv.reader(open(os.path.join(out, "direct_robustness.csv"))))
    reg = list(csv.reader(open(os.path.join(out, "reg_based_robustness.csv"))))
    assert [r[1] for r in direct[-5:]] == names and not any(r[1].startswith("grating_") for r in reg)
    assert len(direct) == 1 + 30 + 5
    lines = list(csv.reader(open(os.path.join(out, "grating_response.csv"))))
    grid = H.grating_grid(512, 8)
    periods = sorted(set(g[5] for g in grid))
    assert lines[0] == H.GRATING_CSV_HEADER and [(l[1], int(l[2])) for l in lines[1:]] == [(name, t) for name in names for t in periods]
    assert all(int(l[3]) == sum(1 for g in grid if g[5] == int(l[2])) for l in lines[1:])
    plain = str(tmp_path / "plain")
    assert H.main(["--device-alterations", "--size", "512", "--levels", "5", "--out", plain]) == 0
    assert not os.path.exists(os.path.join(plain, "grating_response.csv"))
    assert open(os.path.join(plain, "direct_robustness.csv")).read() == "".join(open(os.path.join(out, "direct_robustness.csv")).readlines()[:31])
