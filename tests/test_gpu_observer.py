"""The model-observer relation on the device: musica_sim_observer against metrics.channel_responses, bit for bit, on a plane whose side
(137) is no multiple of 4 and barely holds the largest window (133); every byte lane of a row's words by one-hot templates; the
extremes of the int32 range; identities between entry points; what the call must leave alone, the full strings of its refusals, and
the observer rows of a study on its three paths. Everything compared is an integer, or a double computed on the host from equal
integers: no tolerance anywhere."""
import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

C = mp.C
_I32P = C.POINTER(C.c_int32)
M = mp.OUT_MARGIN
N_SIM = 157
NW = N_SIM - 2 * M   # 137 = 4 * 34 + 1 >= 133
SLOT = 2


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _set_out(p, plane, image_index=0):
    """Makes the 8-bit output of an image `plane` ((NW, NW) integers 0 .. 255): graded = (v + 0.5) / 255 inside a margin of zeros."""
    values = np.pad(np.asarray(plane, np.uint8), M)
    p.set_image(mp.IMG_GRADED, 0, ((values + 0.5) / 255.0).astype(np.float32), image_index=image_index)
    out = p.out_pixels(image_index)
    assert np.array_equal(out, plane)
    return out


def _random_bank(rng, half, channels):
    side = 2 * half + 1
    bank = rng.integers(-128, 128, (channels, side, side)).astype(np.int8)
    bank[0, 0, 0], bank[-1, -1, -1] = -128, 127   # the full int8 range, at the window's two far corners
    return bank


def _places(half, nw=NW):
    """Centres of windows of half-side `half`: all four values of (x - half) mod 4 against the top border, and flush against every border
    and in every corner of the plane."""
    lo, hi = half, nw - 1 - half
    xs = sorted({min(lo + k, hi) for k in range(4)} | {hi})
    ys = sorted({lo, min(lo + 2, hi), hi})
    return [(x, y) for y in ys for x in xs]


def _same(got, want, what=None):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert set(g) == {"a", "b", "pixels", "sum_a", "sum_b"}, what
        for side in ("a", "b"):
            assert g[side].dtype == np.int32 and g[side].shape == w[side].shape and np.array_equal(g[side], w[side]), (what, i, side, g[side], w[side])
        assert all(type(g[k]) is int for k in ("pixels", "sum_a", "sum_b")), what
        assert (g["pixels"], g["sum_a"], g["sum_b"]) == (w["pixels"], w["sum_a"], w["sum_b"]), (what, i)
    return True


PLANE_B = np.random.default_rng(21).integers(0, 256, (NW, NW), dtype=np.uint8)
PLANE_A = np.random.default_rng(22).integers(0, 256, (NW, NW), dtype=np.uint8)


@pytest.fixture(scope="module")
def stepped():
    p = _ctx(N_SIM)
    assert p.execute(phantom(N_SIM, 25, noise=4.0)), mp.last_error()
    p.sim_set_reference(SLOT, PLANE_B)
    yield p
    p.cleanup()


def test_mixed_banks_are_bit_identical(stepped):
    p = stepped
    out = _set_out(p, PLANE_A)
    rng = np.random.default_rng(23)
    banks = [_random_bank(rng, 1, 1), _random_bank(rng, 4, 7), _random_bank(rng, 66, 16), _random_bank(rng, 17, 9)]
    views = [(x, y, k) for k, b in enumerate(banks) for x, y in _places(b.shape[1] // 2)]
    views += [views[0], views[-1], (20, 21, 1), (22, 20, 1), (21, 22, 3), (68, 68, 2), (68, 68, 2), (68, 68, 0)]   # repeated and overlapping
    assert {((x - banks[k].shape[1] // 2) % 4, k) for x, _, k in views} == {(r, k) for r in range(4) for k in range(4)}
    want = H.channel_responses(out, PLANE_B, views, banks)
    assert _same(p.sim_observer(views, banks, SLOT), want, "all in one call")
    for i in (0, len(_places(1)) + 3, next(i for i, v in enumerate(views) if v[2] == 2), len(views) - 1):   # ... and a view alone
        assert _same(p.sim_observer([views[i][:2] + (0,)], [banks[views[i][2]]], SLOT), want[i:i + 1], ("alone", i))


@pytest.mark.parametrize("half", [1, 4, 5, 66])
def test_every_byte_lane(stepped, half):
    """A template whose only non-zero weight is a 1 at (dx, dy) answers with the pixel at (x + dx, y + dy): every column of a row's first
    and of its last, ragged word (S = 3, 9, 11, 133: tails of 3, 1, 3 and 1 bytes), the window's borders, at each alignment."""
    p = stepped
    out = _set_out(p, PLANE_A)
    side = 2 * half + 1
    last = 4 * ((side - 1) // 4)
    cols = sorted(set(range(min(4, side))) | set(range(last, side)) | {half})
    rows = [0, half, side - 1]
    offsets = [(c - half, r - half) for r in rows for c in cols][:mp.OBSERVER_MAX_CHANNELS]
    offsets[-1] = (half, half)   # the far corner whatever was cut
    bank = np.zeros((len(offsets), side, side), np.int8)
    for j, (dx, dy) in enumerate(offsets):
        bank[j, dy + half, dx + half] = 1
    views = [(x, y, 0) for x, y in _places(half)]
    got = p.sim_observer(views, [bank], SLOT)
    for (x, y, _), g in zip(views, got):
        assert g["a"].tolist() == [int(out[y + dy, x + dx]) for dx, dy in offsets], (x, y)
        assert g["b"].tolist() == [int(PLANE_B[y + dy, x + dx]) for dx, dy in offsets], (x, y)


def test_extremes_do_not_wrap(stepped):
    p = stepped
    white = np.full((NW, NW), 255, np.uint8)
    _set_out(p, white)
    p.sim_set_reference(3, white)
    side = 2 * mp.OBSERVER_MAX_HALF + 1
    bank = np.empty((mp.OBSERVER_MAX_CHANNELS, side, side), np.int8)
    bank[0::2], bank[1::2] = -128, 127
    lo, hi = -128 * 255 * side * side, 127 * 255 * side * side
    assert (side, lo, hi) == (133, -577368960, 572858265) and -2 ** 31 <= lo and hi < 2 ** 31
    for g in p.sim_observer([(66, 66, 0), (70, 70, 0), (66, 70, 0)], [bank], 3):
        assert g["a"].tolist() == g["b"].tolist() == [lo, hi] * (mp.OBSERVER_MAX_CHANNELS // 2)
        assert (g["pixels"], g["sum_a"], g["sum_b"]) == (side * side, 255 * side * side, 255 * side * side)


def test_identities_between_entry_points(stepped):
    p = stepped
    out = _set_out(p, PLANE_A)
    rng = np.random.default_rng(24)
    bank = rng.integers(-127, 128, (9, 35, 35)).astype(np.int8)
    views = [(x, y, 0) for x, y in _places(17)]
    plus, minus = p.sim_observer(views, [bank], SLOT), p.sim_observer(views, [-bank], SLOT)
    for (x, y, _), g, h in zip(views, plus, minus):   # negated weights, negated responses; the plain sums are the window's
        assert np.array_equal(g["a"], -h["a"]) and np.array_equal(g["b"], -h["b"]) and g["a"].any()
        assert g["sum_a"] == h["sum_a"] == int(out[y - 17:y + 18, x - 17:x + 18].astype(np.int64).sum())
        assert g["sum_b"] == int(PLANE_B[y - 17:y + 18, x - 17:x + 18].astype(np.int64).sum())
    details = [(10, 10, 1, 0), (30, 12, 2, 0), (70, 60, 8, 0), (NW - 5, NW - 5, 1, 0)]   # the disc channel is musica_sim_details' disc
    v, banks = H.observer_views(details)
    assert [b.shape for b in banks] == [(7, 9, 9), (7, 13, 13), (7, 37, 37)]
    for g, d in zip(p.sim_observer(v, banks, SLOT), p.sim_details(details, SLOT)):
        assert (int(g["a"][-1]), int(g["b"][-1])) == (d["disc"]["sum_a"], d["disc"]["sum_b"])
        assert g["pixels"] == d["box_pixels"]


def test_image_index_reads_its_own_image():
    p = _ctx(N_SIM, batch=2)
    assert p.execute(np.stack([phantom(N_SIM, 30 + k, noise=4.0) for k in range(2)])), mp.last_error()
    outs = [_set_out(p, plane, k) for k, plane in enumerate((PLANE_A, PLANE_A[::-1].copy()))]
    p.sim_set_reference(SLOT, PLANE_B)
    rng = np.random.default_rng(25)
    banks = [_random_bank(rng, 4, 7), _random_bank(rng, 66, 16)]
    views = [(x, y, 0) for x, y in _places(4)] + [(x, y, 1) for x, y in _places(66)]
    got = [p.sim_observer(views, banks, SLOT, image_index=k) for k in range(2)]
    for k in range(2):
        assert _same(got[k], H.channel_responses(outs[k], PLANE_B, views, banks), k)
    assert not np.array_equal(got[0][0]["a"], got[1][0]["a"])
    p.cleanup()


def _call(lib, handle, banks, views, slot=SLOT, image_index=0, extra=0, fill=0x5A5A5A5A):
    """musica_sim_observer itself: (rc, results' bytes, tables with `extra` sentinel words behind them, the words)."""
    barr = (mp.ChannelBank * len(banks))(*[mp.ChannelBank(b.shape[1] // 2, b.shape[0], b.ctypes.data_as(C.POINTER(C.c_int8))) for b in banks])
    varr = (mp.View * len(views))(*[mp.View(*v) for v in views])
    words = sum(2 * banks[k].shape[0] for _, _, k in views)
    res, tables = (mp.SimObserverResult * len(views))(), np.full(words + extra, fill, np.uint32).view(np.int32)
    rc = lib.musica_sim_observer(handle, image_index, slot, len(banks), barr, len(views), varr, res, tables.ctypes.data_as(_I32P), words)
    return rc, bytes(res), tables, words


def test_the_call_only_reads_and_repeats(stepped):
    p = stepped
    _set_out(p, PLANE_A)
    lib = mp.load_library()
    rng = np.random.default_rng(26)
    banks = [_random_bank(rng, 4, 7), _random_bank(rng, 66, 16), _random_bank(rng, 17, 9)]
    views = [(x, y, k) for k, b in enumerate(banks) for x, y in _places(b.shape[1] // 2)]
    out, graded, slot, inp = p.out_pixels(), p.graded().copy(), p.sim_get_reference(SLOT), p.input_pixels().copy()
    runs = []
    for _ in range(2):
        rc, res, tables, words = _call(lib, p._h, banks, views, extra=3)
        assert rc == 1, mp.last_error()
        runs.append((res, tables.tobytes()))
        assert (tables.view(np.uint32)[words:] == 0x5A5A5A5A).all()   # nothing behind the tables
    assert runs[0] == runs[1]
    assert tables[:words].tobytes() == np.concatenate([np.concatenate([w["a"], w["b"]]) for w in H.channel_responses(out, slot, views, banks)]).tobytes()
    assert np.array_equal(p.out_pixels(), out) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(SLOT), slot)
    assert np.array_equal(p.input_pixels(), inp)


def test_refusals_by_their_full_strings():
    p = _ctx(N_SIM)
    lib = mp.load_library()
    assert p.execute(phantom(N_SIM, 25, noise=4.0))
    out = _set_out(p, PLANE_A)
    p.sim_set_reference(SLOT, PLANE_B)
    rng = np.random.default_rng(27)
    bank = _random_bank(rng, 4, 7)
    good = [(3 + 4, 70, 0), (NW - 5, NW - 5, 0)]
    want = H.channel_responses(out, PLANE_B, good, [bank])
    wp = bank.ctypes.data_as(C.POINTER(C.c_int8))
    res = (mp.SimObserverResult * 2)()
    sentinel = bytes(res)
    tables = np.full(64, 0x5A5A5A5A, np.uint32).view(np.int32)
    tp = tables.ctypes.data_as(_I32P)
    graded, slot, inp = p.graded().copy(), p.sim_get_reference(SLOT), p.input_pixels().copy()

    def bank_of(half=4, channels=7, weights=wp):
        return (mp.ChannelBank * 1)(mp.ChannelBank(half, channels, weights))

    def view(*v):
        return (mp.View * 1)(mp.View(*v))

    def refused(text, handle=p._h, idx=0, slot=SLOT, bank_count=1, banks=bank_of(), count=1, views=view(70, 70, 0), results=res, tabs=tp, words=64):
        assert lib.musica_sim_observer(handle, idx, slot, bank_count, banks, count, views, results, tabs, words) == 0
        assert mp.last_error() == "musica_sim_observer: " + text
        assert bytes(res) == sentinel and (tables.view(np.uint32) == 0x5A5A5A5A).all()   # nothing written
        assert _same(p.sim_observer(good, [bank], SLOT), want, text)                     # and a good call goes through behind it

    null = "banks, views, results or tables is NULL"
    refused("ctx is NULL", handle=None)
    refused(null, banks=None)
    refused(null, views=None)
    refused(null, results=None)
    refused(null, tabs=None)
    refused("bank 0: weights is NULL", banks=bank_of(weights=None))
    refused("bank_count 0 out of range [1, 8]", bank_count=0)
    refused("bank_count 9 out of range [1, 8]", bank_count=9)
    refused("count 0 out of range [1, 1024]", count=0)
    refused("count 1025 out of range [1, 1024]", count=1025)
    refused("bank 0: half 0 out of range [1, 66]", banks=bank_of(half=0))
    refused("bank 0: half 67 out of range [1, 66]", banks=bank_of(half=67))
    refused("bank 0: channels 0 out of range [1, 16]", banks=bank_of(channels=0))
    refused("bank 0: channels 17 out of range [1, 16]", banks=bank_of(channels=17))
    refused("view 0: bank 1 is not below 1", views=view(70, 70, 1))
    for x, y in ((3, 70), (70, 3), (NW - 4, 70), (70, NW - 4), (-1, 70), (70, 2 ** 31 - 1)):
        refused("view 0: the window (%d, %d) +- 4 leaves the %d x %d plane" % (x, y, NW, NW), views=view(x, y, 0))
    refused("slot %d >= %d" % (mp.SIM_SLOTS, mp.SIM_SLOTS), slot=mp.SIM_SLOTS)
    refused("slot 5 was never written", slot=5)
    refused("image_index 1 >= batch 1", idx=1)
    refused("table_words 13 is less than the 14 words of the tables", words=13)
    refused("table_words 0 is less than the 14 words of the tables", words=0)
    small = _ctx(2 * M)
    assert lib.musica_sim_observer(small._h, 0, SLOT, 1, bank_of(), 1, view(70, 70, 0), res, tp, 64) == 0
    assert mp.last_error() == "musica_sim_observer: image too small for the 10-pixel margin"
    small.cleanup()
    # the binding refuses before the library, as view_list does
    for views, banks in (([], [bank]), (good, []), ([(3, 70, 0)], [bank]), ([(70, 70, 1)], [bank]), (good, [bank[:, :, :8]]), (good, [np.zeros((17, 9, 9), np.int8)]),
                         (good, [bank.astype(np.float32)]), (good, [bank.astype(np.int16) * 2])):
        with pytest.raises(ValueError):
            p.sim_observer(views, banks, SLOT)
    with pytest.raises(RuntimeError):
        p.sim_observer(good, [bank], 5)
    # after the last refusal a valid call still matches, exactly enough room is enough, and nothing was touched
    assert lib.musica_sim_observer(p._h, 0, SLOT, 1, bank_of(), 1, view(*good[0]), res, tp, 14) == 1, mp.last_error()
    assert tables[:14].tolist() == want[0]["a"].tolist() + want[0]["b"].tolist() and (tables.view(np.uint32)[14:] == 0x5A5A5A5A).all()
    assert (res[0].table_offset, res[0].pixels, res[0].sum_a, res[0].sum_b) == (0, 81, want[0]["sum_a"], want[0]["sum_b"])
    assert np.array_equal(p.input_pixels(), inp) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(SLOT), slot)
    p.cleanup()


# ---- the study -------------------------------------------------------------------------------------------------------------------------
def test_study_rows_agree_on_the_three_paths():
    n = 160
    raw = phantom(n, 11, noise=4.0)
    grid = H.detail_grid(n, 64, radii=(1, 2))
    args = dict(shutters=[], translations=[20], rotations=[], sigmas=[], factors=[], details=[grid])
    runs = {}
    for mode in ("host", "device_metrics", "device_alterations"):
        for observer in (False, True):
            runner = H.Runner(n, 4, device_metrics=mode == "device_metrics", device_alterations=mode == "device_alterations")
            runs[mode, observer] = H.run_study(raw, runner, rng=np.random.default_rng(5), **args, **({"observer": True} if observer else {}))
            runner.close()
        plain, rows = runs[mode, False], runs[mode, True]
        # without the option the rows are those of a study that never heard of it; with it nothing but the new key is added
        assert all("observer" not in r for r in plain), mode
        assert [{k: v for k, v in r.items() if k != "observer"} for r in rows] == plain, mode
        assert list(plain[0]) == ["alteration", "direct", "registered", "mean_cnr", "details"], mode
        assert list(rows[0]) == ["alteration", "direct", "registered", "mean_cnr", "details", "observer"], mode
    host = runs["host", True]
    assert [r["alteration"] for r in host] == ["unaltered", "t_x_20", "t_y_20", "cd_64"]
    for mode in ("device_metrics", "device_alterations"):
        assert [r["observer"] for r in runs[mode, True]] == [r["observer"] for r in host], mode
    assert all(r["observer"] is None for r in host[:-1])
    seen = host[-1]["observer"]["radii"]
    counts = {r: sum(1 for d in grid if d[2] == r) for r in (1, 2)}
    assert list(seen) == [1, 2] and all(set(seen[r]) == set(H.OBSERVER_KEYS) and seen[r]["count"] == counts[r] for r in seen)
    assert all(len(seen[r]["channel_snr"]) == H.OBSERVER_CHANNELS for r in seen)
