"""The exact rational zoom on the device (kernels_zoom.hip): musica_alter_zoom and musica_sim_zoom_reference against harness.zoom bit
for bit (planes below a tile, a last tile 2 wide, odd sides, whole dwords; the widest source window and the strongest zoom beside the
study's five), what they must leave alone, that they repeat, that they commute with the square's symmetries on the device, their
refusals, and the zoom_* rows of a study on its three paths.

Nothing here asserts how far MUSICA is from commuting with magnification: the similarities of a zoom_* row are findings, not
premises."""
import csv
import os

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import harness as H
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

TOL = 1e-12   # what the similarity tests hold between the device metrics and numpy's
# (32, 31): the widest source window of a tile and the largest D; (32, 1): a tile is made from a handful of source pixels
ZOOMS = H.ZOOMS + ((32, 31), (32, 1))


def _ctx(n, levels=4, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=levels, batch=batch), mp.last_error()
    return p


def _full_range_u16(n, seed):
    a = np.random.default_rng(seed).integers(0, 65536, (n, n), dtype=np.uint16)
    a[0, 0], a[-1, -1] = 0, 65535
    a[0, -1], a[-1, 0] = 65535, 0
    assert a.min() == 0 and a.max() == 65535
    return a


def _full_range_u8(nw, seed):
    a = np.random.default_rng(seed).integers(0, 256, (nw, nw), dtype=np.uint8)
    a[0, 0], a[-1, -1] = 0, 255
    a[0, -1], a[-1, 0] = 255, 0
    return a


def _crafted(n, dtype):
    """Constant top value (the largest sum), a 0 / top checkerboard (every weight pair meets the largest step), the ramp (the numerators
    themselves), impulses at the corners, at an edge's middle, at the centre and beside a tile corner."""
    top = np.iinfo(dtype).max
    planes = {"constant": np.full((n, n), top, dtype)}
    i, j = np.indices((n, n))
    planes["checkerboard"] = (((i + j) & 1) * top).astype(dtype)
    planes["ramp"] = ((j * 64) % (top + 1)).astype(dtype)
    for name, (y, x) in (("corner", (0, 0)), ("far corner", (n - 1, n - 1)), ("other corner", (0, n - 1)), ("edge", (0, n // 2)),
                         ("right edge", (n // 2, n - 1)), ("centre", (n // 2, n // 2)), ("tile corner", (64, 63))):
        planes[name] = np.zeros((n, n), dtype)
        planes[name][y, x] = top
    return planes


# 44: below the 64-pixel tile; 130: the last tile is 2 wide; 137: odd; 136: whole dwords, edge tiles 8 wide
@pytest.mark.parametrize("n", [44, 130, 137, 136])
def test_alter_zoom_is_bit_identical(n):
    raw = _full_range_u16(n, n)
    p = _ctx(n)
    p.alter_set_source(raw)
    for z in ZOOMS:
        p.alter_zoom(z)
        assert np.array_equal(p.input_pixels()[0], H.zoom(raw, z)), (n, z)
    if n == 136:
        for name, plane in _crafted(n, np.uint16).items():
            p.alter_set_source(plane)
            for z in ZOOMS:
                p.alter_zoom(z)
                assert np.array_equal(p.input_pixels()[0], H.zoom(plane, z)), (name, z)
    p.cleanup()


def test_only_the_named_image_is_written():
    """N^2 odd: image 1 of the input buffer starts on a 2-byte boundary only; the neighbours on both sides keep every pixel, and so
    does every result of the last step."""
    n = 201
    raw = _full_range_u16(n, 2)
    p = _ctx(n, batch=3)
    base = np.stack([_full_range_u16(n, 20 + k) for k in range(3)])
    assert p.execute(base), mp.last_error()
    graded, out = p.graded().copy(), p.out_pixels(1).copy()
    p.alter_set_source(raw)
    for z in ZOOMS:
        p.alter_zoom(z, image_index=1)
        got = p.input_pixels()
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2]), z
        assert np.array_equal(got[1], H.zoom(raw, z)), z
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.out_pixels(1), out)
    p.cleanup()


# slot sides N - 20: 44 (below a tile), 130 (last tile 2 wide), 137 (odd), 64 (one whole tile)
@pytest.mark.parametrize("n", [64, 150, 157, 84])
def test_zoom_reference_is_bit_identical(n):
    nw = n - 2 * mp.OUT_MARGIN
    plane, other = _full_range_u8(nw, n), _full_range_u8(nw, n + 1)
    p = _ctx(n)
    p.sim_set_reference(0, plane)
    p.sim_set_reference(7, other)
    first = ZOOMS[:6]                        # slots 1 .. 6; the seventh zoom follows into slot 1
    for k, z in enumerate(first):
        p.sim_zoom_reference(1 + k, 0, z)
        assert np.array_equal(p.sim_get_reference(1 + k), H.zoom(plane, z)), (n, z)
        assert np.array_equal(p.sim_get_reference(0), plane) and np.array_equal(p.sim_get_reference(7), other), (n, z)
    for k, z in enumerate(first):            # a later call changed none of the earlier destinations
        assert np.array_equal(p.sim_get_reference(1 + k), H.zoom(plane, z)), (n, z)
    p.sim_zoom_reference(1, 0, ZOOMS[6])
    assert np.array_equal(p.sim_get_reference(1), H.zoom(plane, ZOOMS[6])), (n, ZOOMS[6])
    p.sim_zoom_reference(6, 3, (3, 2))      # a zoomed slot is a source like any other
    assert np.array_equal(p.sim_get_reference(6), H.zoom(H.zoom(plane, ZOOMS[2]), (3, 2)))
    for k in (2, 3, 4, 5):
        assert np.array_equal(p.sim_get_reference(k), H.zoom(plane, ZOOMS[k - 1])), (n, k)
    assert np.array_equal(p.sim_get_reference(0), plane) and np.array_equal(p.sim_get_reference(7), other)
    p.cleanup()


def test_zoom_reference_of_crafted_planes():
    """The u8 kernel on the crafted planes, at a slot side of 136 as the u16 one."""
    n = 156
    p = _ctx(n)
    for name, crafted in _crafted(n - 2 * mp.OUT_MARGIN, np.uint8).items():
        p.sim_set_reference(0, crafted)
        for z in ZOOMS:
            p.sim_zoom_reference(1, 0, z)
            assert np.array_equal(p.sim_get_reference(1), H.zoom(crafted, z)), (name, z)
    p.cleanup()


def test_both_entry_points_repeat_bit_for_bit():
    n = 150
    raw = _full_range_u16(n, 5)
    plane = _full_range_u8(n - 20, 6)
    p = _ctx(n)
    p.alter_set_source(raw)
    p.sim_set_reference(0, plane)
    for z in ((21, 20), (32, 1)):
        images, slots = [], []
        for _ in range(2):
            p.alter_none()                  # something else in between
            p.alter_zoom(z)
            images.append(p.input_pixels()[0].copy())
            p.sim_set_reference(1, plane[::-1].copy())
            p.sim_zoom_reference(1, 0, z)
            slots.append(p.sim_get_reference(1).copy())
        assert np.array_equal(images[0], images[1]) and np.array_equal(slots[0], slots[1]), z
    p.cleanup()


def test_zoom_commutes_with_the_symmetries_on_the_device():
    """zoom of a symmetry equals the symmetry of the zoom, every step on the device: slot to slot, and the source plane through the
    input buffer."""
    n, z = 157, (5, 4)
    raw = _full_range_u16(n, 3)
    plane = _full_range_u8(n - 20, 4)
    p = _ctx(n)
    p.sim_set_reference(0, plane)
    p.sim_zoom_reference(1, 0, z)
    for e in (1, 4, 7):
        p.sim_transform_reference(2, 0, e)
        p.sim_zoom_reference(3, 2, z)
        p.sim_transform_reference(4, 1, e)
        assert np.array_equal(p.sim_get_reference(3), p.sim_get_reference(4)), e
        assert np.array_equal(p.sim_get_reference(3), H.apply_symmetry(H.zoom(plane, z), e)), e

        p.alter_set_source(raw)
        p.alter_symmetry(e)
        p.alter_set_source(p.input_pixels()[0].copy())
        p.alter_zoom(z)
        zoom_of_symmetry = p.input_pixels()[0].copy()
        p.alter_set_source(raw)
        p.alter_zoom(z)
        p.alter_set_source(p.input_pixels()[0].copy())
        p.alter_symmetry(e)
        assert np.array_equal(p.input_pixels()[0], zoom_of_symmetry), e
    p.cleanup()


BAD = ((2, 0), (1, 1), (4, 5), (33, 32), (33, 1), (1 << 20, 1), (4, 2), (30, 24), (0, 0))


def test_refusals_leave_the_context_usable():
    n, levels = 264, 4
    raw = phantom(n, 25, noise=4.0)
    p = _ctx(n, levels)
    lib = mp.load_library()
    assert p.execute(raw)
    p.sim_capture(0)
    p.alter_set_source(raw)
    p.alter_none()
    graded, slot0, inp = p.graded().copy(), p.sim_get_reference(0), p.input_pixels().copy()

    def refused(rc, words):
        assert rc == 0
        msg = mp.last_error()
        assert words in msg, msg

    for bp, bq in BAD:
        refused(lib.musica_alter_zoom(p._h, 0, bp, bq), "zoom")
        refused(lib.musica_sim_zoom_reference(p._h, 1, 0, bp, bq), "zoom")
        with pytest.raises(ValueError):
            p.alter_zoom((bp, bq))
        with pytest.raises(ValueError):
            p.sim_zoom_reference(1, 0, (bp, bq))
    refused(lib.musica_alter_zoom(p._h, 1, 2, 1), "image_index")           # image_index == batch
    refused(lib.musica_alter_zoom(None, 0, 2, 1), "NULL")
    refused(lib.musica_sim_zoom_reference(None, 1, 0, 2, 1), "NULL")
    refused(lib.musica_sim_zoom_reference(p._h, 0, 0, 2, 1), "dst_slot == src_slot")
    refused(lib.musica_sim_zoom_reference(p._h, 1, 5, 2, 1), "never written")
    refused(lib.musica_sim_zoom_reference(p._h, mp.SIM_SLOTS, 0, 2, 1), "slot")
    refused(lib.musica_sim_zoom_reference(p._h, 1, mp.SIM_SLOTS, 2, 1), "slot")
    fresh = _ctx(n, levels)
    refused(lib.musica_alter_zoom(fresh._h, 0, 2, 1), "no source")
    small = _ctx(2 * mp.OUT_MARGIN)                                         # too small for the margin: no slot can ever be written
    refused(lib.musica_sim_zoom_reference(small._h, 1, 0, 2, 1), "never written")
    small.cleanup()
    # nothing was touched by the refused calls: no image, no result, no slot; slot 1 is still unwritten
    assert np.array_equal(p.input_pixels(), inp) and np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    with pytest.raises(RuntimeError):
        p.sim_get_reference(1)
    # a successful zoom of either kind changes neither the last step's results nor the source slot ...
    p.alter_zoom((5, 4))
    p.sim_zoom_reference(1, 0, (5, 4))
    assert np.array_equal(p.graded(), graded) and np.array_equal(p.sim_get_reference(0), slot0)
    assert np.array_equal(p.sim_get_reference(1), H.zoom(slot0, (5, 4)))
    # ... and the step on the resident buffer processes what the alteration wrote
    assert p.execute_device()
    p.sync()
    assert fresh.execute(H.zoom(raw, (5, 4)))
    assert np.array_equal(p.graded(), fresh.graded())
    assert np.array_equal(p.input_pixels()[0], H.zoom(raw, (5, 4)))
    # the whole frame is the region of a registered comparison
    res = p.sim_compare([(0, 1) + H.roi_zoom(slot0.shape)])[0]
    assert res["pixels"] == (n - 20) ** 2
    p.cleanup()
    fresh.cleanup()


def _close(a, b, what):
    """Two study rows' values: floats to TOL, everything else (ints, None, lists of them, dicts) exactly alike. Returns the largest
    difference of a float."""
    worst = 0.0
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), what
        for k in a:
            worst = max(worst, _close(a[k], b[k], what + (k,)))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            worst = max(worst, _close(x, y, what + (i,)))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    elif isinstance(a, float):
        if a != b:
            print(what, a, b, abs(a - b))
        assert abs(a - b) <= TOL, (what, a, b)
        worst = abs(a - b)
    else:
        assert a == b, (what, a, b)
    return worst


def test_study_rows_agree_on_the_three_paths(tmp_path):
    n, levels = 276, 4
    zooms = H.ZOOMS[:2]
    raw = phantom(n, 11, noise=4.0)
    args = dict(shutters=H.scaled(H.SHUTTERS, n)[:1], translations=H.scaled(H.TRANSLATIONS, n)[:1], rotations=[9], sigmas=[], factors=[],
                symmetries=(4,), blurs=(2,), tone=True, scales=3, displacement=3)
    studies, full = {}, {}
    for name, kw in (("host", {}), ("metrics", dict(device_metrics=True)), ("alterations", dict(device_alterations=True))):
        runner = H.Runner(n, levels, **kw)
        rows = full[name] = H.run_study(raw, runner, rng=np.random.default_rng(5), zooms=zooms, **args)
        plain = H.run_study(raw, runner, rng=np.random.default_rng(5), **args)
        runner.close()
        names = [r["alteration"] for r in rows]
        assert names[len(plain) - 2:] == ["d4_4", "blur_2", "zoom_21_20", "zoom_11_10"], name      # the rows follow the d4 and blur rows
        assert not any(r["alteration"].startswith("zoom_") for r in plain), name
        assert rows[:len(plain)] == plain, name           # every other row is the row of the study without zooms
        studies[name] = rows[len(plain):]
        for r in studies[name]:
            assert list(r) == list(plain[-1]), (name, r["alteration"])
            assert all(v is not None for v in r.values()), (name, r["alteration"])   # the whole frame is always registered
    assert studies["alterations"] == studies["metrics"]   # the zoomed image is the host's bit for bit: every number, and mean_cnr, exactly
    for h, d in zip(studies["host"], studies["metrics"]):
        assert h["alteration"] == d["alteration"] and h["mean_cnr"] == d["mean_cnr"]
        worst = _close(h, d, (h["alteration"],))
        print(h["alteration"], "largest difference between the host's and the device's floats", worst)
    # the CSV tables take the rows up like any other
    out = str(tmp_path / "out")
    H.write_studies_csvs([("phantom", full["alterations"])], out)
    for table in ("direct_robustness.csv", "reg_based_robustness.csv", "mean_cnr.csv", "tone_robustness.csv", "displacement.csv",
                  "scale_robustness.csv"):
        lines = list(csv.reader(open(os.path.join(out, table))))
        assert [r[1] for r in lines[-2:]] == ["zoom_21_20", "zoom_11_10"], table
        assert all(cell != "" for r in lines[-2:] for cell in r[:4]), table
        assert sum(r[1].startswith("zoom_") for r in lines) == 2, table
