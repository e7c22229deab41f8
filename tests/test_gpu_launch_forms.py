"""The launch forms the timed path runs, held to the oracle where they take effect.

  * the timed form itself: three MUSICA_FLAG_LINEAR contexts of a musica_pipeline at bench.py's 8 x 2048^2 / L6, the library's
    defaults (sdev inside the expand launches, the paired launches k_rb_sdev of the one-stream script);
  * the pair geometry: chains of 0 .. 4 pairs, a chain cut short by the one-launch tail of small levels, both forms of the sdev role
    (one run per workgroup, the row march), the plain and the swizzled role_tile, batches (blockIdx.z image indexing);
  * the plain tile mappings (MUSICA_XCD_SWIZZLE=0, MUSICA_XCD_REGIONS=0), read once per context;
  * the debug surface of a context that does not store its sdev images: injected band images must not change the step's sdev images.

Every comparison is bit-exact against ob.Oracle(..., ORDER_FAST) (test_gpu_parity.py states the bars).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom
from test_gpu_baseline_configs import _check_both
from test_gpu_parity import _compare_all, _proc, _same

pytestmark = pytest.mark.gpu


def _phantoms(n, seeds):
    """Seeded phantoms on a few host threads (each depends on its seed alone)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    with ThreadPoolExecutor(max(1, min(len(seeds), cores, 16))) as ex:
        return np.stack(list(ex.map(lambda s: phantom(n, s), seeds)))


def _library_defaults(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MUSICA_"):
            monkeypatch.delenv(k)


def test_timed_pipeline_form_at_its_size(ob, monkeypatch):
    """What bench.py times: musica_pipeline_* with three contexts of 8 x 2048^2 / L6 and nothing overridden. Each context computes sdev inside
    its expand launches and runs four pairs (the sdev pass of level i with reduce + band of level i + 1, i = 0 .. 3). Context 0 holds the
    rank-0 shard (seeds 100 .. 107), the others other images; after six steps (every context replays its graph twice) every image of every
    context is the oracle's, and context 0's are the committed digests."""
    _library_defaults(monkeypatch)
    n, levels, b, depth = 2048, 6, 8, 3
    seeds = [[100 + k for k in range(b)], [200 + k for k in range(b)], [300 + k for k in range(b)]]
    px = [_phantoms(n, s) for s in seeds]
    pipe = mp.MusicaPipeline(n, levels=levels, batch=b, depth=depth)
    pipe.upload(px[0])
    pipe.prime()
    ctx = [pipe.context(c) for c in range(depth)]
    for c in range(depth):
        assert ctx[c].dispatch() == (1, True)
        assert ctx[c].fuses_sdev()
        assert ctx[c].paired_levels() == 4
        ctx[c].upload(px[c])
    for _ in range(2 * depth):
        pipe.step()
    pipe.sync()
    for c in range(depth):
        for k in range(b):
            o = ob.Oracle(n, levels, ob.ORDER_FAST).execute(px[c][k])
            _compare_all(ctx[c], o, ob, idx=k, tag="context %d image %d: " % (c, k))
            if c == 0:
                _check_both(ctx[c], k, o, ob, "2048_L6_s%d_f0" % seeds[c][k], False)
    pipe.cleanup()


_RUN = {"MUSICA_AUTOTUNE": "0", "MUSICA_SDEV_RUN": "1"}                              # the sdev role: one 16-row run per workgroup
_MARCH = {"MUSICA_AUTOTUNE": "0", "MUSICA_SDEV_RUN": "0", "MUSICA_SDEV_ROWS": "16"}  # the sdev role: 16-row marches
# side, levels, pairs one step runs: 1032 (1032, 516: level 1 is not a multiple of 8) pairs nothing; 1040, 1056, 1088, 1152 chain 1 .. 4 pairs
# (level 0's run form at 1040: 65 workgroups per strip, the plain role_tile; at 1152: 72, the swizzled one); 256 / 512 at the reference's
# level rule stop at 3 pairs because the tiny tail starts at level 4 (T = 4). Two cases per row, every batch / sdev form / role form
# against every other and against every row.
_GEOMETRY = [
    (1032, 6, 0, 1, "0", _RUN), (1032, 6, 0, 3, "1", _MARCH),
    (1040, 6, 1, 1, "1", _RUN), (1040, 6, 1, 3, "0", _MARCH),
    (1056, 6, 2, 1, "0", _MARCH), (1056, 6, 2, 3, "1", _RUN),
    (1088, 6, 3, 1, "1", _MARCH), (1088, 6, 3, 3, "0", _RUN),
    (1152, 6, 4, 1, "0", _RUN), (1152, 6, 4, 3, "1", _MARCH),
    (256, 0, 3, 1, "1", _RUN), (256, 0, 3, 3, "0", _MARCH),
    (512, 0, 3, 1, "0", _MARCH), (512, 0, 3, 3, "1", _RUN),
    (1152, 6, 4, 1, "0", dict(_RUN, MUSICA_XCD_SWIZZLE="0")),   # the plain role_tile where the swizzled one would apply
]


@pytest.mark.parametrize("n,levels,pairs,batch,sd,env", _GEOMETRY,
                         ids=["%d_L%d_b%d_sd%s_%s%s" % (c[0], c[1], c[3], c[4], "run" if c[5]["MUSICA_SDEV_RUN"] == "1" else "march",
                                                       "_noswz" if "MUSICA_XCD_SWIZZLE" in c[5] else "") for c in _GEOMETRY])
def test_paired_launch_geometry(ob, n, levels, pairs, batch, sd, env, monkeypatch):
    """Lone one-stream contexts with the pairs on: the number of pairs a step runs, and every image of every batch member against the oracle."""
    _library_defaults(monkeypatch)
    monkeypatch.setenv("MUSICA_STREAMS", "1")
    monkeypatch.setenv("MUSICA_PAIR_RB_SDEV", "1")
    monkeypatch.setenv("MUSICA_SDEV_IN_EXPAND", sd)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    px = np.stack([phantom(n, 7 * n + 3 * levels + k) for k in range(batch)])
    p = _proc(n, levels, batch=batch)
    assert p.dispatch()[0] == 1
    assert p.fuses_sdev() == (sd == "1")
    assert p.paired_levels() == pairs
    assert p.execute(px), mp.last_error()
    for k in range(batch):
        o = ob.Oracle(n, levels, ob.ORDER_FAST).execute(px[k])
        _compare_all(p, o, ob, idx=k, tag="%d / L%d image %d: " % (n, levels, k))
    p.cleanup()


def test_paired_levels_is_zero_where_no_pair_runs(monkeypatch):
    """Pairing off, two streams, or the generic kernels: no step runs a pair."""
    _library_defaults(monkeypatch)
    monkeypatch.setenv("MUSICA_PAIR_RB_SDEV", "0")
    monkeypatch.setenv("MUSICA_STREAMS", "1")
    p = _proc(1152, 6)
    assert p.paired_levels() == 0
    p.cleanup()
    monkeypatch.setenv("MUSICA_PAIR_RB_SDEV", "1")
    monkeypatch.setenv("MUSICA_STREAMS", "2")
    p = _proc(1152, 6)
    assert p.dispatch()[0] == 2 and p.paired_levels() == 0
    p.cleanup()
    monkeypatch.setenv("MUSICA_STREAMS", "1")
    p = _proc(1152, 6, flags=mp.FLAG_GENERIC_KERNELS)
    assert p.paired_levels() == 0
    p.cleanup()


@pytest.mark.parametrize("side,batch,env", [(4096, 2, {"MUSICA_XCD_SWIZZLE": "0"}), (4096, 2, {"MUSICA_XCD_REGIONS": "0"}),
                                            (1536, 2, {"MUSICA_XCD_SWIZZLE": "0"})],
                         ids=["4096_noswz", "4096_noregions", "1536_noswz"])
def test_metric_kernel_with_the_plain_tile_mappings(ob, side, batch, env, monkeypatch):
    """The metric kernel (k_reduce_dma) with the 2-D regions (4096: 8 strips) or the swizzled xcd_tile (1536: 3 strips, 192 grid rows)
    switched off for the context: the plain mapping, bit-identical to the oracle."""
    _library_defaults(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(side + 1)
    img = rng.random((batch, side, side), dtype=np.float32)
    p = _proc(64, 4)
    got = p.k_reduce_host(img)
    for k in range(batch):
        _same(got[k], ob.k_downsample(ob.k_smooth(img[k], ob.ORDER_FAST)), "smooth+downsample side %d image %d %s" % (side, k, env))
    p.cleanup()


@pytest.mark.parametrize("sd", ["0", "1"])
def test_injected_band_images_leave_the_steps_sdev_images(ob, sd, monkeypatch):
    """musica_debug_set_image(BANDPASS) after a step, then the debug surface, on a context that stores its sdev images (sd = 0) and on one
    that computes them inside the expand launches (sd = 1) and produces them on demand. Both keep the step's sdev images, as the oracle
    does: the sdev getter right after the injection, and the expand stage (which reads the injected bands and the step's sdev)."""
    _library_defaults(monkeypatch)
    monkeypatch.setenv("MUSICA_SDEV_IN_EXPAND", sd)
    n, levels = 1024, 6
    px = phantom(n, 77)
    o = ob.Oracle(n, levels, ob.ORDER_FAST).execute(px)
    lit = ob.Oracle(n, levels, ob.ORDER_REFERENCE).execute(px)
    bands = [lit.image(ob.IMG_BANDPASS, i) for i in range(4)]
    assert not np.array_equal(bands[0], o.image(ob.IMG_BANDPASS, 0))   # the injection changes the band: the sdev computed from it would differ
    p = _proc(n, levels)
    assert p.fuses_sdev() == (sd == "1")
    assert p.execute(px), mp.last_error()
    for i in range(4):
        p.set_image(mp.IMG_BANDPASS, i, bands[i])
        o.set_image(ob.IMG_BANDPASS, i, bands[i])
    for i in range(4):
        _same(p.image(mp.IMG_SDEV, i), o.image(ob.IMG_SDEV, i), "sdev[%d] after the injection" % i)
    p.run_stage(mp.STAGE_EXPAND)
    o.run_stage(ob.STAGE_EXPAND)
    for i in range(levels):
        _same(p.image(mp.IMG_EXPAND, i), o.image(ob.IMG_EXPAND, i), "expand[%d]" % i)
    for i in range(4):
        _same(p.image(mp.IMG_EXP_BANDPASS, i), o.image(ob.IMG_EXP_BANDPASS, i), "exp_bandpass[%d]" % i)
        _same(p.image(mp.IMG_CONTRAST_BAND, i), o.image(ob.IMG_CONTRAST_BAND, i), "contrast_band[%d]" % i)
    p.cleanup()
