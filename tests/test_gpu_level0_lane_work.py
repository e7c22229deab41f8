"""The level-0 marches do edge-lane work only on the lanes that use it; everything they store or bin stays the oracle's, bit for bit.

Changes of which lanes or wavefronts execute an expression (never of the expression) are pinned here:
  B  reduce + band of the raw level normalises its four halo pixels on four lanes of the strip's edge quad, one each, and gathers their
     vertical chains back with quad broadcasts;
  C  the sdev march and the expand launch's sdev window carry one edge pair per lane (left on lane 0, right on lane 63) and the DPP moves
     leave it where the neighbour lane does not exist;
  A  (measured in round 6 and not kept; the inputs stay for whoever tries again) the level-0 expand launch skipping bin,
     weight and LDS add of the gradation histogram (and the CLAHE add) for a row outside the 100-pixel border and for a row pair in which no
     lane of the wavefront sits under a cnr texel with a relevance weight, while the exact-zero test (gradation_histogram.comp:24) still
     sees every texel. The launch bins every texel today; these inputs are the ones on which a skip can go wrong.

Bars: test_gpu_parity.py's — every image bit-identical, every histogram, curve and scalar equal.

Shapes, the smallest at which each lever can go wrong:
  520 / L4            two strips, the second 8 columns wide: the image's last lane is lane 0 of its strip
  1040 / L5           512 + 512 + 16: an interior strip with halos on both sides; levels 0 and 1 are multiples of 8
  1536 / L6, batch 2  three full strips, blockIdx.z
  2048 / L6           the smallest side whose CLAHE histogram is counted inside the expand launch (tile side >= a strip): one image

Inputs for A are crafted, and what they decide is asserted on the ORACLE's cnr, relevant and reconstruction images before the device is
judged (_facts): a 64-texel cnr segment is what one wavefront's 512 columns sit under for four row pairs, and it is `skipped` when no
texel of it that owns a column inside the border has a weight by classify_cnr (kernels_common.h), `binned` otherwise — every segment
is one or the other. _facts also asserts what the skip rests on: under a skipped segment the oracle's relevant image has no pixel with
uint(relevant * 100) != 0 and none with relevant == 1.0 (the CLAHE histogram's condition)."""
import os

import numpy as np
import pytest

import noise_hist_restatement as R
import test_gpu_noise_breaks as NB
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom
from test_gpu_parity import _compare_all, _proc, _same

pytestmark = pytest.mark.gpu

f32 = np.float32
BORDER = 100          # img_relevant.comp:46-49
STRIP = 512           # columns of a wavefront's strip, 8 per lane


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _flat_half(n):
    """Flat rows on top, a phantom in the middle, black below: skipped segments above and below binned ones, exact zeros of the
    reconstruction deep inside the black part — inside the border rows and in the border rows at the bottom."""
    px = phantom(n, 7)
    px[:(3 * n) // 8] = 30000
    px[(9 * n) // 16:] = 0
    return px


def _noisy_patch(n):
    """A flat image with one 32 x 32 patch of noise left of the border columns: the cnr it raises reaches the first lanes that own a column
    inside the border and fades out there, so some segment has a single lane with a weight. No exact zero anywhere."""
    px = np.full((n, n), 30000, dtype=np.uint16)
    px[n // 2:n // 2 + 32, 40:72] = np.random.default_rng(5).integers(20000, 40000, size=(32, 32))
    return px


def _collimator(n):
    """tests/noise_hist_restatement.crafted_raw: stamps all over a phantom and a black frame — every segment is binned."""
    return R.crafted_raw(phantom(n, 500), 0)


def _ramp(n):
    """Every uint16 value (n * n >= 65536): the linear index modulo 65536, so neighbouring columns differ across every strip edge."""
    return (np.arange(n * n, dtype=np.uint32) & 0xFFFF).astype(np.uint16).reshape(n, n)


def _ramp_down(n):
    """The same ramp running along the columns and downwards, times 257: large steps between the halo columns."""
    return ((np.arange(n * n, dtype=np.uint32).reshape(n, n).T[::-1] * 257) & 0xFFFF).astype(np.uint16).copy()


def _flat(n):
    return np.full((n, n), 30000, dtype=np.uint16)      # min == max: den == 0


_IMAGES = {"flat_half": _flat_half, "noisy_patch": _noisy_patch, "collimator": _collimator, "ramp": _ramp, "ramp_down": _ramp_down, "flat": _flat}
_WANT = {}     # (n, levels, name, oracle flags) -> (pixels, executed oracle, facts): built once, only read afterwards


def _texel_has_weight(cnr):
    """classify_cnr on a cnr image: w_cnr or w_dark_or_ramp of the texel is non-zero (ramp with uint(r^5 * 100) >= 1, or high)."""
    c = cnr * f32(256.0)
    with np.errstate(invalid="ignore"):
        ramp = (c >= 1) & (c <= 6)
        high = (c >= 6) & (c <= 256)
        r = c / f32(6.0)
        r2 = r * r
        w = np.where(ramp, ((r2 * r2) * r) * f32(100.0), f32(0)).astype(np.uint32)
    return (ramp & (w >= 1)) | high


def _facts(o, ob, n):
    """What an image decides, from the oracle's images alone. Segments are counted over the cnr rows whose 8 pixel rows all lie inside the
    border rows and the strips that own a column inside the border."""
    nz = _texel_has_weight(o.image(ob.IMG_CNR, 3))
    rec, rel = o.image(ob.IMG_EXPAND, 0), o.image(ob.IMG_RELEVANT)
    zero = rec == 0
    cols = np.arange(n)
    col_in = (cols > BORDER) & (cols < n - BORDER)
    lanes = nz[:, :n // 8] & col_in.reshape(-1, 8).any(axis=1)[None, :]
    rows = n // 8
    row_in = [8 * r > BORDER and 8 * r + 7 < n - BORDER for r in range(rows)]
    f = dict(skipped=0, binned=0, zero_in_skipped=0, skipped_above_binned=0, skipped_below_binned=0, single_lane=0,
             zeros=int(zero.sum()), zeros_in_border_rows=int(zero[:BORDER + 1].sum() + zero[n - BORDER:].sum()))
    for s in range((n + STRIP - 1) // STRIP):
        c0, c1 = STRIP * s, min(STRIP * s + STRIP, n)
        if not col_in[c0:c1].any():
            continue
        cnt = lanes[:, c0 // 8:c1 // 8].sum(axis=1)
        for r in range(rows):
            if not row_in[r]:
                continue
            if cnt[r] == 0:
                blk = (slice(8 * r, 8 * r + 8), slice(c0, c1))
                assert ((rel[blk] * f32(100.0)).astype(np.uint32) == 0).all(), "a skipped segment (cnr row %d, strip %d) holds a weighted pixel" % (r, s)
                assert not (rel[blk] == 1.0).any(), "a skipped segment (cnr row %d, strip %d) holds a pixel the CLAHE histogram counts" % (r, s)
                f["skipped"] += 1
                f["zero_in_skipped"] += bool(zero[blk].any())
                f["skipped_above_binned"] += bool(r + 1 < rows and row_in[r + 1] and cnt[r + 1] > 0)
                f["skipped_below_binned"] += bool(r > 0 and row_in[r - 1] and cnt[r - 1] > 0)
            else:
                f["binned"] += 1
                f["single_lane"] += bool(cnt[r] == 1)
    return f


def _want(ob, n, levels, name, oflags=0):
    key = (n, levels, name, oflags)
    if key not in _WANT:
        px = _IMAGES[name](n)
        o = ob.Oracle(n, levels, ob.ORDER_FAST, oflags).execute(px)
        _WANT[key] = (px, o, _facts(o, ob, n))
    return _WANT[key]


def _assert_inputs_decide(ob, n, levels, names, oflags=0):
    """The conditions of lever A, on the oracle. A crafted input that misses one is to be fixed, not the condition."""
    for name in names:
        f = _want(ob, n, levels, name, oflags)[2]
        tag = "%d / L%d %s: %r" % (n, levels, name, f)
        if name == "flat_half":
            assert f["zero_in_skipped"] > 0, tag            # an all-zero segment inside the border rows that holds an exact zero
            assert f["skipped_above_binned"] > 0 and f["skipped_below_binned"] > 0, tag
            assert f["zeros_in_border_rows"] > 0, tag
        elif name == "noisy_patch":
            assert f["single_lane"] > 0 and f["skipped"] > 0, tag
            assert f["zeros"] == 0, tag                     # an image without any zero keeps the fused count
        elif name == "collimator":
            assert f["skipped"] == 0 and f["binned"] > 0, tag


def _env(monkeypatch, **env):
    NB._library_defaults(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compare_key_outputs(p, o, ob, idx, tag):
    _same(p.image(mp.IMG_BANDPASS, 0, idx), o.image(ob.IMG_BANDPASS, 0), tag + "bandpass[0]")
    _same(p.image(mp.IMG_DOWNSAMPLED, 1, idx), o.image(ob.IMG_DOWNSAMPLED, 1), tag + "downsampled[1]")
    _same(p.image(mp.IMG_SDEV, 0, idx), o.image(ob.IMG_SDEV, 0), tag + "sdev[0]")
    assert np.array_equal(p.noise_hist(0, idx), o.noise_hist(0)), tag + "noise_hist[0]"
    _same(p.image(mp.IMG_EXPAND, 0, idx), o.image(ob.IMG_EXPAND, 0), tag + "expand[0]")
    assert np.array_equal(p.grad_hist(idx), o.grad_hist()), tag + "grad_hist"
    gc, gw = p.grad_curve(idx)
    oc, ow = o.grad_curve()
    assert np.array_equal(gc, oc) and gw == ow, tag + "grad_curve"
    _same(p.image(mp.IMG_GRADED, 0, idx), o.image(ob.IMG_GRADED), tag + "graded")


def _step_case(ob, n, levels, names, flags, sd, monkeypatch, oflags=0):
    """The batch `names` through a context of the given form: captured graph (everything compared) and eager launches (the level-0 outputs)."""
    px = np.stack([_want(ob, n, levels, name, oflags)[0] for name in names])
    for graph in ("1", "0"):
        _env(monkeypatch, MUSICA_SDEV_IN_EXPAND=sd, MUSICA_GRAPH=graph)
        p = _proc(n, levels, batch=len(names), flags=flags)
        assert p.fuses_gradhist(), "the gradation histogram is not counted by the level-0 expand launch at %d / L%d" % (n, levels)
        assert p.fuses_sdev() == (sd == "1")
        for rep in range(2):                                # the second execute replays what the first set up; gzero is re-armed per execute
            assert p.execute(px), mp.last_error()
        for k, name in enumerate(names):
            o = _want(ob, n, levels, name, oflags)[1]
            tag = "%d / L%d flags %d sd %s graph %s, %s: " % (n, levels, flags, sd, graph, name)
            if graph == "1":
                _compare_all(p, o, ob, idx=k, tag=tag)
            else:
                _compare_key_outputs(p, o, ob, k, tag)
        p.cleanup()


_SHAPES = [(520, 4, ("flat_half", "collimator", "noisy_patch")), (1040, 5, ("flat_half", "collimator", "noisy_patch")), (1536, 6, ("flat_half", "noisy_patch"))]
_SHAPE_IDS = ["%d_L%d" % s[:2] for s in _SHAPES]
_CONTEXTS = {"lone": 0, "linear": mp.FLAG_LINEAR}


@pytest.mark.parametrize("sd", ["1", "0"])
@pytest.mark.parametrize("form", list(_CONTEXTS))
@pytest.mark.parametrize("n,levels,names", _SHAPES, ids=_SHAPE_IDS)
def test_gradation_histogram_is_binned_only_where_a_weight_can_be_non_zero(ob, n, levels, names, form, sd, monkeypatch):
    """Lever A's inputs: skipped and binned segments one above the other, a segment with a single weighted lane, exact zeros inside skipped
    segments (inside the border rows and in the border rows) that must still raise gzero and send the image to the literal recount,
    next to an image of the same batch without a zero that keeps the fused count."""
    _assert_inputs_decide(ob, n, levels, names)
    _step_case(ob, n, levels, names, _CONTEXTS[form], sd, monkeypatch)


def test_clahe_histogram_is_skipped_with_the_gradation_histogram(ob, monkeypatch):
    """CH on board (2048 / L6, one image): no CLAHE add exists where both weights are 0 — _facts asserts that on the oracle's relevant
    image — so the skipped rows lose nothing of clahe_histogram.comp either."""
    n, levels, names = 2048, 6, ("flat_half",)
    _assert_inputs_decide(ob, n, levels, names, ob.FLAG_CLAHE)
    f = _want(ob, n, levels, "flat_half", ob.FLAG_CLAHE)[2]
    assert f["single_lane"] > 0 and f["binned"] > 0
    px, o, _ = _want(ob, n, levels, "flat_half", ob.FLAG_CLAHE)
    assert int(o.clahe_hist().sum()) > 0
    _env(monkeypatch, MUSICA_SDEV_IN_EXPAND="1", MUSICA_CLAHE_IN_EXPAND="1")
    p = _proc(n, levels, flags=mp.FLAG_CLAHE)
    assert p.fuses_gradhist() and p.fuses_sdev()
    for rep in range(2):
        assert p.execute(px[None]), mp.last_error()
    _compare_all(p, o, ob, tag="clahe, flat half: ")
    assert np.array_equal(p.clahe_hist(), o.clahe_hist())
    a, b = p.clahe_curves(), o.clahe_curves()
    assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()
    _same(p.image(mp.IMG_CLAHE_GRADED), o.image(ob.IMG_CLAHE_GRADED), "clahe graded")
    p.cleanup()


_EDGE_SHAPES = [(520, 4, ("ramp", "flat", "ramp_down")), (1040, 5, ("ramp", "flat", "ramp_down")), (1536, 6, ("ramp", "ramp_down"))]


@pytest.mark.parametrize("sd", ["1", "0"])
@pytest.mark.parametrize("form", list(_CONTEXTS))
@pytest.mark.parametrize("n,levels,names", _EDGE_SHAPES, ids=_SHAPE_IDS)
def test_halo_and_edge_columns_across_strip_edges(ob, n, levels, names, form, sd, monkeypatch):
    """Levers B and C: every uint16 value in ramps whose halo columns differ from their neighbours at every strip edge, and a flat image
    (den == 0: the oracle defines the outcome). Band, coarse, sdev, noise histograms and everything downstream against the oracle; with
    sd = 1 the expand launches' sdev window, with sd = 0 the sdev march, in lone and one-stream contexts (the paired launch's roles)."""
    _step_case(ob, n, levels, names, _CONTEXTS[form], sd, monkeypatch)


@pytest.mark.parametrize("form", ["march16", "run", "default"])
@pytest.mark.parametrize("n,levels", [(520, 4), (1040, 5), (1536, 6)], ids=_SHAPE_IDS)
def test_sdev_edge_columns_on_crafted_band_images(ob, n, levels, form, monkeypatch):
    """Lever C on band images injected through set_image(BANDPASS): tests/noise_hist_restatement.crafted_bands puts its dead patches on the
    first and the last lane of every strip, where a lane's 5 x 5 sums take the shared edge pair. A batch of two, a different image per slot."""
    env, flags, order = NB._FORMS[form]
    NB._run_stage_case(ob, n, levels, env, flags, order, (0, 1), monkeypatch)
