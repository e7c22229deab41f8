"""The refusals of the five table comparisons (musica_sim_profiles / _levels / _gradients / _order / _reach), word for word: every refusal
that the calls' own tests (test_gpu_gain, _levels, _gradients, _order, _reach) provoke, at the sides those tests use, and a few double
refusals that pin which of two comes first, against the complete musica_last_error() strings recorded in
golden/table_call_refusals.json by golden/make_table_call_refusals.py. The neighbours look for a keyword per refusal; a reworded or
reordered message shows here. Every call is refused on its arguments, before any device work."""
import json
import os

import numpy as np
import pytest

from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd import processing as mp
from metamorphic_testing_of_the_musica_algorithm_for_x_ray_image_processing_amd.phantom import phantom

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_call_refusals.json")
SIDE, SIDE_REACH = 264, 84          # the contexts of the neighbours' refusal tests
SENTINEL = 0xDEADBEEF
_U64P = mp.C.POINTER(mp.C.c_uint64)


def _ctx(n, batch=1):
    p = mp.MusicaProcessing(device=0)
    assert p.init(n, levels=4, batch=batch), mp.last_error()
    return p


def _query(*q):
    return (mp.SimQuery * 1)(mp.SimQuery(*q))


def _radii(*v):
    return np.array(v, np.uint32)


class _Call:
    """One of the five calls: its largest count, result type, table words, smallest side, and the words a query's table takes."""

    def __init__(self, name, most, result, dtype, min_side, per, lead=()):
        self.name, self.most, self.min_side, self.per, self.lead = name, most, min_side, per, lead
        self.res = (result * (most + 1))()
        self.ptr = mp._U32P if dtype == np.uint32 else _U64P
        self.dtype = dtype
        self.many = (mp.SimQuery * (most + 1))(*[mp.SimQuery(0, 0, 0, 0, 0, 0, 8, 8)] * (most + 1))
        self.good = _query(0, 0, 3, 4, 3, 4, 9, 8)

    def room(self, nw):
        self.tables = np.full(self.most * self.per(nw, nw), SENTINEL, self.dtype)

    def __call__(self, h, count, qs, res, tables, table_words, lead=None):
        """The library's answer and its message. res, tables: True for the call's own arrays, None for NULL."""
        lead = self.lead if lead is None else lead
        keep = [a for a in lead if isinstance(a, np.ndarray)]               # alive over the call
        args = [a.ctypes.data_as(mp._U32P) if isinstance(a, np.ndarray) else a for a in lead]
        rc = getattr(mp.load_library(), self.name)(h, *args, count, qs, self.res if res else None,
                                                   self.tables.ctypes.data_as(self.ptr) if tables else None, table_words)
        del keep
        return rc, mp.last_error()


def _calls():
    return [_Call("musica_sim_profiles", mp.PROFILE_MAX_QUERIES, mp.SimProfileResult, np.uint32, 1, lambda w, h: 4 * (w + h)),
            _Call("musica_sim_levels", mp.LEVEL_MAX_QUERIES, mp.SimLevelResult, np.uint64, 1, lambda w, h: 4096 * 6, (4,)),
            _Call("musica_sim_gradients", mp.SIM_MAX_QUERIES, mp.SimGradientResult, np.uint64, 7, lambda w, h: 22 * 6),
            _Call("musica_sim_order", mp.SIM_MAX_QUERIES, mp.SimOrderResult, np.uint64, 7, lambda w, h: mp.ORDER_TABLE_WORDS),
            _Call("musica_sim_reach", mp.REACH_MAX_QUERIES, mp.SimReachResult, np.uint64, 1, lambda w, h: 3 * 6, (2, _radii(0, 5)))]


def refusals():
    """{case: the complete message} of every refused call, in the order they are made."""
    got = {}

    def refused(call, case, h, count, qs, res=True, tables=True, table_words=None, lead=None):
        rc, msg = call(h, count, qs, res, tables, call.tables.size if table_words is None else table_words, lead)
        assert rc == 0, "%s / %s was not refused" % (call.name, case)
        assert call.name + " / " + case not in got
        got[call.name + " / " + case] = msg

    def common(call, p, nw):
        """What every one of the five refuses alike, on a context with slot 0 written (and a source plane where the call needs one)."""
        h, good, many, words = p._h, call.good, call.many, call.per(nw, nw)
        full = _query(0, 0, 0, 0, 0, 0, nw, nw)
        refused(call, "ctx NULL", None, 1, good)
        refused(call, "queries NULL", h, 1, None)
        refused(call, "results NULL", h, 1, good, res=False)
        refused(call, "tables NULL", h, 1, good, tables=False)
        refused(call, "count 0", h, 0, many)
        refused(call, "count above the most", h, call.most + 1, many)
        refused(call, "slot out of range", h, 1, _query(0, mp.SIM_SLOTS, 0, 0, 0, 0, 8, 8))
        refused(call, "slot never written", h, 1, _query(0, 5, 0, 0, 0, 0, 8, 8))
        refused(call, "image_index == batch", h, 1, _query(1, 0, 0, 0, 0, 0, 8, 8))
        low = call.min_side - 1
        refused(call, "w below the smallest side", h, 1, _query(0, 0, 0, 0, 0, 0, low, 8))
        refused(call, "h below the smallest side", h, 1, _query(0, 0, 0, 0, 0, 0, 8, low))
        s = call.min_side
        e = nw - s + 1                                                      # the first origin at which the smallest region leaves
        for k, q in enumerate(((0, 0, e, 0, 0, 0, s, s), (0, 0, 0, e, 0, 0, s, s), (0, 0, 0, 0, e, 0, s, s), (0, 0, 0, 0, 0, e, s, s),
                               (0, 0, 1, 0, 0, 0, nw, s), (0, 0, 0, 0, 0, 1, s, nw), (0, 0, 0, 0, 0, 0, 1 << 31, 1 << 31))):
            refused(call, "region leaves the plane %d" % k, h, 1, _query(*q))
        refused(call, "table_words one short", h, 1, full, table_words=words - 1)
        refused(call, "table_words 0", h, 1, full, table_words=0)
        refused(call, "table_words one short of two queries", h, 2, many, table_words=2 * call.per(8, 8) - 1)
        # two refusals at once: which comes first
        refused(call, "count 0 and tables NULL", h, 0, many, tables=False)
        refused(call, "bad query and short table_words", h, 1, _query(0, mp.SIM_SLOTS, 0, 0, 0, 0, 8, 8), table_words=0)

    profiles, levels, gradients, order, reach = calls = _calls()
    raw = phantom(SIDE, 25, noise=4.0)
    nw = SIDE - 2 * mp.OUT_MARGIN
    for call in calls[:4]:
        call.room(nw)
    p = _ctx(SIDE)
    assert p.execute(raw), mp.last_error()
    for call in calls[:4]:
        refused(call, "slot 0 never written", p._h, 1, call.good)          # a context that captured nothing
    p.sim_capture(0)
    refused(levels, "no source plane", p._h, 1, levels.good)
    p.alter_set_source(raw)
    for call in calls[:4]:
        common(call, p, nw)
    refused(levels, "shift below the least", p._h, 1, levels.good, lead=(3,))
    refused(levels, "shift above the most", p._h, 1, levels.good, lead=(16,))
    refused(levels, "table_words 0 at shift 8", p._h, 1, levels.good, table_words=0, lead=(8,))
    refused(levels, "bad shift and tables NULL", p._h, 1, levels.good, tables=False, lead=(16,))
    small = _ctx(2 * mp.OUT_MARGIN)
    for call in calls[:4]:
        refused(call, "no plane inside the margin", small._h, 1, call.good)
    p.cleanup()

    # the reach, at its own test's side; two images for the refusals about the pair of input and output
    raw = np.stack([phantom(SIDE_REACH, 30 + k, noise=4.0) for k in range(2)])
    nw = SIDE_REACH - 2 * mp.OUT_MARGIN
    reach.room(nw)
    p = _ctx(SIDE_REACH)
    assert p.execute(raw[0]), mp.last_error()
    refused(reach, "slot 0 never written", p._h, 1, reach.good)
    p.sim_capture(0)
    refused(reach, "no source plane", p._h, 1, reach.good)
    p.alter_set_source(raw[0])
    common(reach, p, nw)
    for case, lead in (("radii NULL", (2, None)), ("radii_count 0", (0, _radii(0, 5))), ("radii_count above the most", (33, _radii(*range(33)))),
                       ("radii[0] not 0", (2, _radii(1, 5))), ("radii equal", (3, _radii(0, 5, 5))), ("radii descend", (3, _radii(0, 5, 4))),
                       ("radius above the most", (2, _radii(0, 16384)))):
        refused(reach, case, p._h, 1, reach.good, lead=lead)
    refused(reach, "radii NULL and tables NULL", p._h, 1, reach.good, tables=False, lead=(2, None))
    refused(reach, "no plane inside the margin", small._h, 1, reach.good)
    small.cleanup()
    p.cleanup()
    p, other = _ctx(SIDE_REACH, batch=2), _ctx(SIDE_REACH, batch=2)
    assert p.execute(raw), mp.last_error()
    p.alter_set_source(raw[0])
    p.sim_capture(0)
    pair = (mp.SimQuery * 2)(mp.SimQuery(0, 0, 0, 0, 0, 0, 9, 9), mp.SimQuery(1, 0, 0, 0, 0, 0, 9, 9))
    refused(reach, "two image indices", p._h, 2, pair)
    refused(reach, "two image indices and short table_words", p._h, 2, pair, table_words=0)
    other.upload(raw)
    assert p.execute_device(other.input_device_ptr()), mp.last_error()
    p.sync()
    refused(reach, "the last step's input is not the context's", p._h, 1, reach.good)
    other.cleanup()
    p.cleanup()
    for call in calls:
        assert (call.tables == SENTINEL).all(), call.name                   # no refused call wrote a word of the tables
    return got


def test_every_refusal_reads_as_recorded():
    want = json.load(open(GOLDEN))["refusals"]
    got = refusals()
    assert list(got) == list(want)                                           # the same cases
    for case in want:
        assert got[case] == want[case], case
