"""The tone-table relation on the device: musica_alter_lut against harness.apply_lut and musica_sim_levels against
harness.level_statistics, bit for bit, at the sides where the kernels take another path; the flush rule of k_sim_levels at the smallest
size at which a workgroup counts more than a u32 word holds; what both must leave alone, their refusals, and the lut rows of a study on
its three paths. Every comparison is of integers, or of floats that one host function made of equal integers: exact throughout."""
import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

_U64P = mp.C.POINTER(mp.C.c_uint64)
IDENTITY = np.arange(65536, dtype=np.uint16)


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _full_range_u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    a[0, -1], a[-1, 0] = 65535, 0
    a[1, 1], a[2, 2] = 1, 65534
    return a


def _tables(raw, seed):
    """Random tables, the identity, a constant, a permutation and every fourth spec of LUTS."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 65536, 65536), rng.integers(0, 65536, 65536), IDENTITY, np.full(65536, 4711), rng.permutation(65536)] + \
           [lut for _, lut in H.LUTS(raw)[::4]]


def _check(p, raw, lut, image_index=0):
    p.alter_lut(lut, image_index)
    got = p.input_pixels()[image_index].copy()
    assert np.array_equal(got, H.apply_lut(raw, lut))
    return got


# 84: 84^2 % 8 = 0, 16-byte words; 137: odd, single pixels; 90: 90^2 % 8 = 4, dwords only
@pytest.mark.parametrize("n", [84, 137, 90])
def test_alter_lut_is_bit_identical(n):
    raw = _full_range_u16(n, n)
    p = _ctx(n)
    p.alter_set_source(raw)
    for lut in _tables(raw, n):
        _check(p, raw, lut)
    assert np.array_equal(_check(p, raw, IDENTITY), raw)                          # the identity copies
    assert (_check(p, raw, np.full(65536, 4711)) == 4711).all()
    p.cleanup()


# 1160: 168 200 16-byte chunks, 42 workgroups of 4096 chunks, the last ragged; 1025: odd, 1 050 625 single pixels, more than the 256
# workgroups take in one round: the first take a second, ragged, group
@pytest.mark.parametrize("n", [1160, 1025])
def test_alter_lut_over_several_workgroups(n):
    raw = _full_range_u16(n, 4)
    p = _ctx(n)
    p.alter_set_source(raw)
    rng = np.random.default_rng(6)
    _check(p, raw, rng.integers(0, 65536, 65536))
    _check(p, raw, rng.permutation(65536))
    _check(p, raw, H.LUTS(raw)[-1][1])
    p.cleanup()


def test_only_the_named_image_is_written():
    """N^2 odd: image 1 of the input buffer starts on a 2-byte boundary only; the neighbours on both sides keep every pixel."""
    n = 201
    raw = _full_range_u16(n, 2)
    p = _ctx(n, batch=3)
    base = np.stack([_full_range_u16(n, 20 + k) for k in range(3)])
    p.upload(base)
    p.alter_set_source(raw)
    for lut in _tables(raw, 1)[:4]:
        p.alter_lut(lut, image_index=1)
        got = p.input_pixels()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2])
        assert np.array_equal(got[1], H.apply_lut(raw, lut))
    p.cleanup()


# ---- the levels ------------------------------------------------------------------------------------------------------------------------
N_SIM = 320
NW_SIM = N_SIM - 2 * mp.OUT_MARGIN
FULL = (0, 0, 0, 0, NW_SIM, NW_SIM)
# the full frame, 1 x 1 at a corner, different origins on the two sides across tile borders at odd offsets, one line
REGIONS = [FULL, (NW_SIM - 1, NW_SIM - 1, 0, 0, 1, 1), (61, 3, 5, 9, 131, 193), (7, 299, 0, 7, 293, 1)]
assert len(REGIONS) == mp.LEVEL_MAX_QUERIES
SHIFTS = (4, 8, 15)                                                               # 4096, 256 and 2 classes


def _set_out(p, values, image_index=0):
    """Makes the 8-bit output of an image `values` ((N, N) integers 0 .. 255; the margin is cropped): graded = (v + 0.5) / 255."""
    p.set_image(mp.IMG_GRADED, 0, ((np.asarray(values) + 0.5) / 255.0).astype(np.float32), image_index=image_index)
    m = mp.OUT_MARGIN
    out = p.out_pixels(image_index)
    assert np.array_equal(out, np.asarray(values)[m:-m, m:-m])
    return out


def _same(got, want, classes):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == {"table", "classes", "ssd", "pixels"} and g["classes"] == classes
        assert g["table"].dtype == np.uint64 and g["table"].shape == (classes, 6) and np.array_equal(g["table"], w)
        assert type(g["ssd"]) is int and g["ssd"] == int(w[:, 3].sum()) and type(g["pixels"]) is int and g["pixels"] == int(w[:, 0].sum())
    return True


def _queries(regions, slot, image_index=0):
    return [(image_index, slot) + tuple(r) for r in regions]


def _outputs(n):
    rng = np.random.default_rng(8)
    random = rng.integers(0, 256, (n, n), dtype=np.uint8)
    random[mp.OUT_MARGIN, mp.OUT_MARGIN], random[-mp.OUT_MARGIN - 1, -mp.OUT_MARGIN - 1] = 0, 255
    return {"random": random, "white": np.full((n, n), 255, np.uint8), "zero": np.zeros((n, n), np.uint8)}


SOURCES = {"random": _full_range_u16(N_SIM, 12), "flat": np.full((N_SIM, N_SIM), 51234, np.uint16)}   # flat: every pixel in one class, the most contended case
PLANES = {2: np.random.default_rng(9).integers(0, 256, (NW_SIM, NW_SIM), dtype=np.uint8), 3: np.zeros((NW_SIM, NW_SIM), np.uint8)}


@pytest.fixture(scope="module")
def stepped():
    p = _ctx(N_SIM)
    assert p.execute(phantom(N_SIM, 25, noise=4.0)), mp.last_error()
    for slot, plane in PLANES.items():
        p.sim_set_reference(slot, plane)
    yield p
    p.cleanup()


@pytest.mark.parametrize("name", ["random", "white", "zero"])
def test_sim_levels_is_bit_identical(stepped, name):
    p = stepped
    out = _set_out(p, _outputs(N_SIM)[name])
    for source, raw in SOURCES.items():
        p.alter_set_source(raw)
        for shift in SHIFTS:
            count = mp.level_count(shift)
            classes = H.level_classes(raw, shift)
            for slot, plane in PLANES.items():
                want = H.level_statistics(out, plane, classes, REGIONS, count)
                assert _same(p.sim_levels(_queries(REGIONS, slot), shift), want, count), (name, source, shift, slot)   # four queries in one call
                assert _same(p.sim_levels(_queries(REGIONS[2:3], slot), shift), want[2:3], count), (name, source, shift, slot)   # ... and one alone
    if name == "white":                                                           # all 255 against all 0 in one class: the largest sums
        got = p.sim_levels(_queries([FULL], 3), 15)[0]
        px = NW_SIM * NW_SIM
        assert got["table"][1].tolist() == [px, 255 * px, 0, 65025 * px, 65025 * px, 0] and not got["table"][0].any() and got["ssd"] == 65025 * px
    for r in REGIONS:                                                             # ssd is the compare call's integer
        if min(r[4], r[5]) >= 7:
            res = p.sim_compare(_queries([r], 2))[0]
            got = p.sim_levels(_queries([r], 2), 8)[0]
            assert got["ssd"] == res["sq_diff_sum"] and got["pixels"] == res["pixels"], r


def test_sim_levels_returns_identical_bytes_twice(stepped):
    p = stepped
    _set_out(p, _outputs(N_SIM)["random"])
    p.alter_set_source(SOURCES["random"])
    lib = mp.load_library()
    qs = [mp.SimQuery(*q) for q in _queries(REGIONS, 2)]
    arr = (mp.SimQuery * len(qs))(*qs)
    for shift in SHIFTS:
        count = mp.level_count(shift)
        words = len(qs) * count * 6
        runs = []
        for _ in range(2):
            res, tables = (mp.SimLevelResult * len(qs))(), np.full(words + 3, 0xDEADBEEF, np.uint64)
            assert lib.musica_sim_levels(p._h, shift, len(qs), arr, res, tables.ctypes.data_as(_U64P), words) == 1, mp.last_error()
            runs.append((bytes(res), tables.tobytes()))
        assert runs[0] == runs[1]
        assert (tables[words:] == 0xDEADBEEF).all()                               # nothing behind the tables is written
        for i, (r, q) in enumerate(zip(res, REGIONS)):                            # the tables lie one behind the other, every word written
            assert (r.table_offset, r.classes, r.pixels) == (i * count * 6, count, q[4] * q[5])
    p.sim_capture(6)
    assert all(d["ssd"] == 0 and not d["table"][:, 3].any() and np.array_equal(d["table"][:, 1], d["table"][:, 2])
               for d in p.sim_levels(_queries([FULL, (13, 27, 13, 27, 131, 77)], 6), 4))   # the output against itself


def test_sim_levels_reads_the_named_image_and_slot():
    n = 137
    nw = n - 2 * mp.OUT_MARGIN
    p = _ctx(n, batch=2)
    assert p.execute(np.stack([phantom(n, 30 + k, noise=4.0) for k in range(2)])), mp.last_error()
    raw = _full_range_u16(n, 7)
    p.alter_set_source(raw)
    planes = {5: np.random.default_rng(1).integers(0, 256, (nw, nw), dtype=np.uint8), 6: np.random.default_rng(2).integers(0, 256, (nw, nw), dtype=np.uint8)}
    for slot, plane in planes.items():
        p.sim_set_reference(slot, plane)
    regions = [(0, 0, 0, 0, nw, nw), (3, 5, 7, 1, 101, 99), (nw - 1, 0, 0, nw - 1, 1, 1)]      # an odd plane side
    classes = H.level_classes(raw, 8)
    for k in range(2):
        for slot, plane in planes.items():
            assert _same(p.sim_levels(_queries(regions, slot, k), 8), H.level_statistics(p.out_pixels(k), plane, classes, regions, 256), 256), (k, slot)
    mixed = [(k, slot) + regions[1] for k in range(2) for slot in planes]                      # ... and mixed in one call
    want = [H.level_statistics(p.out_pixels(k), planes[slot], classes, regions[1:2], 256)[0] for k in range(2) for slot in planes]
    assert _same(p.sim_levels(mixed, 8), want, 256)
    p.cleanup()


# ---- the flush rule --------------------------------------------------------------------------------------------------------------------
def _most_counted(side, count):
    """The pixels the busiest workgroup of k_sim_levels counts for `count` full-frame queries of a side x side plane, by the launch
    geometry of DESIGN.md section 4 (level_geometry): a query gets 128 // count workgroups; a chunk is max(1, min(65535 // w,
    max(ceil(16384 / w), ceil(h / workgroups)))) rows; workgroup g takes the chunks g, g + workgroups, ...: workgroup 0 counts the most."""
    blocks = 128 // count
    rows = max(1, min(65535 // side, max(-(-16384 // side), -(-side // blocks))))
    chunks = -(-side // rows)
    return sum(min(rows, side - c * rows) * side for c in range(0, chunks, min(chunks, blocks)))


SIDE_FLUSH = 1441


def test_the_flush_rule_where_a_workgroup_counts_more_than_a_word_holds():
    """A 32-bit field of sum (a - b)^2 holds 66 051 pixels of a = 255 against b = 0 (and a 24-bit field of sum a 65 793). With four
    full-frame queries a query has 32 workgroups. Up to a side of 1440 a chunk has ceil(side / 32) rows and every workgroup counts one
    chunk of at most 65 535 pixels. At 1441 that would be 46 rows of 1441 = 66 286 pixels, so a chunk is capped at 65535 // 1441 = 45
    rows (64 845 pixels) and there are 33 of them: workgroup 0 takes chunk 0 and the one-row chunk 32, 66 286 pixels in all, and must
    flush between the two; a kernel that did not would wrap sum_dd and sum_aa of the one class and carry sum_a into sum_b."""
    side = SIDE_FLUSH
    assert min(s for s in range(1, 2100) if _most_counted(s, 4) > 66051) == side and _most_counted(side, 4) == 46 * side == 66286
    assert all(_most_counted(s, 1) <= 65535 for s in range(1, 2850))              # a single query, 128 workgroups, needs a side of 2850
    n = side + 2 * mp.OUT_MARGIN
    full = (0, 0, 0, 0, side, side)
    p = _ctx(n)
    assert p.execute(np.random.default_rng(1).integers(0, 4096, (n, n)).astype(np.uint16)), mp.last_error()
    out = _set_out(p, np.full((n, n), 255, np.uint8))
    p.sim_set_reference(1, np.zeros((side, side), np.uint8))
    p.alter_set_source(np.full((n, n), 40000, np.uint16))                         # one class: 40000 >> 4 = 2500
    got = p.sim_levels(_queries([full] * 4, 1), 4)
    px = side * side
    for g in got:
        assert g["table"][2500].tolist() == [px, 255 * px, 0, 65025 * px, 65025 * px, 0] and g["ssd"] == 65025 * px and g["pixels"] == px
        assert not np.delete(g["table"], 2500, axis=0).any()
    assert np.array_equal(got[0]["table"], H.level_statistics(out, np.zeros((side, side), np.uint8), np.full((side, side), 2500), [full], 4096)[0])
    # ... and the other way round, b = 255 against a = 0: the largest sum b and sum b^2 a workgroup holds
    _set_out(p, np.zeros((n, n), np.uint8))
    p.sim_set_reference(1, np.full((side, side), 255, np.uint8))
    for g in p.sim_levels(_queries([full] * 4, 1), 4):
        assert g["table"][2500].tolist() == [px, 0, 255 * px, 65025 * px, 0, 65025 * px] and not np.delete(g["table"], 2500, axis=0).any()
    p.cleanup()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    n, levels = 264, 4
    nw = n - 2 * mp.OUT_MARGIN
    raw = phantom(n, 25, noise=4.0)
    p = _ctx(n, levels)
    lib = mp.load_library()
    assert p.execute(raw)
    p.sim_capture(0)
    res = (mp.SimLevelResult * (mp.LEVEL_MAX_QUERIES + 1))()
    words = mp.LEVEL_MAX_QUERIES * 4096 * 6
    tables = np.full(words, 0xDEADBEEF, np.uint64)
    tp = tables.ctypes.data_as(_U64P)
    scratch = np.zeros(2 * 6, np.uint64)
    good = (mp.SimQuery * 1)(mp.SimQuery(0, 0, 3, 4, 3, 4, 9, 5))
    lut = np.ascontiguousarray(H.LUTS(raw)[0][1])
    lp = lut.ctypes.data_as(mp._U16P)
    # no source plane yet: both calls say so, and the context goes on
    assert lib.musica_alter_lut(p._h, 0, lp) == 0 and "no source" in mp.last_error()
    assert lib.musica_sim_levels(p._h, 4, 1, good, res, tp, words) == 0 and "no source" in mp.last_error()
    p.alter_set_source(raw)
    p.alter_none()
    graded, slot0, inp = p.graded().copy(), p.sim_get_reference(0), p.input_pixels().copy()

    def refused(rc, text):
        assert rc == 0
        msg = mp.last_error()
        assert text in msg, msg
        # ... and a good call goes through behind every refusal
        assert lib.musica_sim_levels(p._h, 15, 1, good, res, scratch.ctypes.data_as(_U64P), scratch.size) == 1, mp.last_error()
        assert (res[0].classes, res[0].ssd, res[0].pixels) == (2, 0, 45) and int(scratch[0] + scratch[6]) == 45

    def query(*q):
        return (mp.SimQuery * 1)(mp.SimQuery(*q))

    refused(lib.musica_alter_lut(None, 0, lp), "NULL")
    refused(lib.musica_alter_lut(p._h, 0, None), "NULL")
    refused(lib.musica_alter_lut(p._h, 1, lp), "image_index")                     # image_index == batch
    refused(lib.musica_sim_levels(None, 4, 1, good, res, tp, words), "NULL")
    refused(lib.musica_sim_levels(p._h, 4, 1, None, res, tp, words), "NULL")
    refused(lib.musica_sim_levels(p._h, 4, 1, good, None, tp, words), "NULL")
    refused(lib.musica_sim_levels(p._h, 4, 1, good, res, None, words), "NULL")
    refused(lib.musica_sim_levels(p._h, 3, 1, good, res, tp, words), "shift")
    refused(lib.musica_sim_levels(p._h, 16, 1, good, res, tp, words), "shift")
    many = (mp.SimQuery * (mp.LEVEL_MAX_QUERIES + 1))(*[mp.SimQuery(0, 0, 0, 0, 0, 0, 2, 2)] * (mp.LEVEL_MAX_QUERIES + 1))
    refused(lib.musica_sim_levels(p._h, 4, 0, many, res, tp, words), "count")
    refused(lib.musica_sim_levels(p._h, 4, mp.LEVEL_MAX_QUERIES + 1, many, res, tp, words), "count")
    refused(lib.musica_sim_levels(p._h, 4, 1, query(0, mp.SIM_SLOTS, 0, 0, 0, 0, 8, 8), res, tp, words), "slot")
    refused(lib.musica_sim_levels(p._h, 4, 1, query(0, 5, 0, 0, 0, 0, 8, 8), res, tp, words), "never written")
    refused(lib.musica_sim_levels(p._h, 4, 1, query(1, 0, 0, 0, 0, 0, 8, 8), res, tp, words), "image_index")
    refused(lib.musica_sim_levels(p._h, 4, 1, query(0, 0, 0, 0, 0, 0, 0, 8), res, tp, words), "side")          # the smallest side is 1
    for q in ((0, 0, nw, 0, 0, 0, 1, 1), (0, 0, 0, nw, 0, 0, 1, 1), (0, 0, 0, 0, nw, 0, 1, 1), (0, 0, 0, 0, 0, nw, 1, 1), (0, 0, 1, 0, 0, 0, nw, 1),
              (0, 0, 0, 0, 0, 1, 1, nw), (0, 0, 0, 0, 0, 0, 1 << 31, 1 << 31)):
        refused(lib.musica_sim_levels(p._h, 4, 1, query(*q), res, tp, words), "leaves")
    full = query(0, 0, 0, 0, 0, 0, nw, nw)
    refused(lib.musica_sim_levels(p._h, 4, 1, full, res, tp, 4096 * 6 - 1), "table_words")
    refused(lib.musica_sim_levels(p._h, 8, 1, full, res, tp, 0), "table_words")
    assert (tables == 0xDEADBEEF).all()                                           # no refused call wrote a word of the tables
    assert lib.musica_sim_levels(p._h, 4, 1, full, res, tp, 4096 * 6) == 1        # exactly enough room
    assert (tables[4096 * 6:] == 0xDEADBEEF).all() and res[0].ssd == 0 and res[0].table_offset == 0 and int(tables[:4096 * 6:6].sum()) == nw * nw
    assert lib.musica_sim_levels(p._h, 15, 1, query(0, 0, 5, 5, 5, 5, 1, 1), res, tp, 12) == 1 and res[0].pixels == 1   # a 1 x 1 region is taken
    for bad in (IDENTITY[:-1], np.full(65536, 65536), np.full(65536, -1), np.full(65536, 0.5)):   # the binding refuses before the library
        with pytest.raises(ValueError):
            p.alter_lut(bad)
    for queries, shift in (([], 4), ([(0, 0) + (0, 0, 0, 0, 2, 2)] * 5, 4), ([(0, 0, 0, 0, 0, 0, 2, 2)], 3), ([(0, 0, 0, 0, 0, 0, 2, 2)], 16), ([(0, 0, 0, 0, 0, 0, 2, 2)], 4.0)):
        with pytest.raises(ValueError):
            p.sim_levels(queries, shift)
    fresh = _ctx(n, levels)
    assert lib.musica_sim_levels(fresh._h, 4, 1, good, res, tp, words) == 0 and "never written" in mp.last_error()
    small = _ctx(2 * mp.OUT_MARGIN)
    assert lib.musica_sim_levels(small._h, 4, 1, good, res, tp, words) == 0 and "margin" in mp.last_error()
    small.cleanup()
    # nothing was touched by the refused calls (nor by the measurements that ran): no image, no result, no slot; slot 1 is unwritten
    assert np.array_equal(p.input_pixels(), inp) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    with pytest.raises(RuntimeError):
        p.sim_get_reference(1)
    # a successful table changes neither the last step's results nor a slot ...
    p.alter_lut(lut)
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    assert p.sim_levels([(0, 0, 0, 0, 0, 0, nw, nw)], 4)[0]["ssd"] == 0           # the output is still the captured one
    # ... and the step on the resident buffer processes what the table wrote
    assert p.execute_device()
    p.sync()
    assert fresh.execute(H.apply_lut(raw, lut))
    assert np.array_equal(p.graded(), fresh.graded())
    assert np.array_equal(p.input_pixels()[0], H.apply_lut(raw, lut))
    want = H.level_statistics(fresh.out_pixels(), slot0, H.level_classes(raw, 4), [(0, 0, 0, 0, nw, nw)], 4096)
    assert _same(p.sim_levels([(0, 0, 0, 0, 0, 0, nw, nw)], 4), want, 4096)
    p.cleanup()
    fresh.cleanup()


# ---- the study -------------------------------------------------------------------------------------------------------------------------
def _grids(n):
    return dict(shutters=H.scaled(H.SHUTTERS, n)[:1], translations=H.scaled(H.TRANSLATIONS, n)[:1], rotations=[9], sigmas=[16.0], factors=[0.05])


def _study(n, raw, luts, **runner_args):
    runner = H.Runner(n, 4, **runner_args)
    rows = H.run_study(raw, runner, rng=np.random.default_rng(5), blurs=[1], luts=luts, lut_tables=luts is not None, **_grids(n))
    runner.close()
    return rows


def test_study_rows_agree_on_the_three_paths():
    n = 148
    raw = phantom(n, 11, noise=4.0)
    luts = H.LUTS(raw)[::5]
    names = ["offset_8", "clip_8", "bits_12", "gamma_3_4", "negative"]
    studies = {}
    for name, args in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        rows = _study(n, raw, luts, **args)
        plain = _study(n, raw, None, **args)
        assert [r["alteration"] for r in rows[len(plain):]] == names, name
        # the rows before them are the rows of the study without luts, but for the key: every other key of every row is equal
        assert all(r["levels"] is None for r in rows[:len(plain)]), name
        assert [{k: v for k, v in r.items() if k != "levels"} for r in rows[:len(plain)]] == plain, name
        assert all("levels" not in r for r in plain), name
        studies[name] = rows[len(plain):]
        for r in studies[name]:
            assert set(r) == {"alteration", "mean_cnr", "direct", "registered", "levels"} and r["registered"] is None, (name, r["alteration"])
            d = r["levels"]
            assert set(d) == set(H.LEVEL_KEYS) | {"levels", "curve_a", "curve_b"} and d["classes"] == len(d["levels"]) == len(d["curve_a"]) == len(d["curve_b"])
        assert studies[name][0]["levels"]["levels"] == sorted(int(v) for v in np.unique(H.level_classes(raw, 4)))
    assert studies["alterations"] == studies["metrics"]   # every number of every row, exactly
    for h, d in zip(studies["host"], studies["metrics"]):
        assert h["alteration"] == d["alteration"] and h["mean_cnr"] == d["mean_cnr"]
        assert h["levels"] == d["levels"], h["alteration"]                        # exact integers, one summary: equal to the last bit
