"""The pair span on the device (agx_span.hip, agx_unit_pair_span, agx_unit_walk_span) against tests/span_model.py on the units of
tests/test_span_cases.py: every case of tests/walk_units.py, tests/edge_units.py and tests/lean_units.py and the generated seeds 201 and 203.  Per unit one build serves
every check: pair_span of the whole unit and of the windows of test_span_cases.windows (empty, one position, [63, 65), mid-tile to mid-tile, the last partial tile), field
by field; sub-windows forced to 64 and to 100 positions; a second call; walk_span on the stretches of the unit's own finish and on the hand-made tables (jumps around a
fragment's end, an entry two bases take, a jump nobody spans, steps that are not forward, the jump out of flat base 63, side ids; section 14's tables with ids without a
node) at min_span 0, 1, the model's median span and one above every span; base chunks forced to 64 and 128; tracks of a middle record range; the same per-position answer
after reprune + finish; a unit without edge counters and without kept paths; the refusals; and that the calls plan and hold what an export does and leave the finish's
bytes alone.  Every comparison is integer equality."""
import os

import numpy as np
import pytest

import span_model as SM
from test_gpu_evidence import malformed
from test_span_cases import UNITS, modelled, thresholds, windows  # noqa: F401  (modelled: the module fixture)

pytestmark = pytest.mark.gpu

NAMES = list(UNITS)
NONE = SM.NONE


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def built_unit(agx, m, build=True, **kw):
    u = m["u"]
    flags = dict(keep_counts=True, keep_paths=True)
    flags.update(kw)
    e = agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, **flags)
    e.load_files(m["tmp"], 0)
    e.upload()
    if build:
        e.build()
    return e


def forced(e, env, call, *a, **kw):
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return call(*a, **kw)
    finally:
        for k in env:
            del os.environ[k]


def tables_of(m, w):
    return dict(m["tables"], own=w)


def run_engine(agx, m):
    """One build of the unit; everything the tests look at, collected before the unit goes."""
    u, n_pos = m["u"], m["n_pos"]
    out = {}
    with built_unit(agx, m) as e:
        out["need"] = e.hbm_needed()
        out["fin"] = e.finish()
        w = out["w"] = e.walk_paths()
        e.unitigs()
        out["stats0"] = e.stats()
        out["pair"] = {win: e.pair_span(win) for win in windows(n_pos)}
        out["whole"] = e.pair_span()
        out["again"] = e.pair_span()
        out["sub"] = {(c, win): forced(e, {"AGX_SPAN_CHUNK": c}, e.pair_span, win) for c in (64, 100) for win in (None, windows(n_pos)[4])}
        out["stats1"] = e.stats()
        out["based"] = {k: SM.bases(m["front"], m["side_xpos"], t, m["frags"]) for k, t in tables_of(m, w).items()}
        out["ts"] = {k: thresholds(m, b) for k, b in out["based"].items()}
        out["walk"] = {(k, t): e.walk_span(tab, t, tracks=True) for k, tab in tables_of(m, w).items() for t in out["ts"][k]}
        out["default"] = e.walk_span(min_span=2)
        out["chunks"] = {(c, k, t): forced(e, {"AGX_SPAN_BASE_CHUNK": c, "AGX_SPAN_CHUNK": 100}, e.walk_span, tab, t, tracks=True)
                         for c in (64, 128) for k, tab in tables_of(m, w).items() for t in out["ts"][k][2:]}
        nr = len(w["rec_len"])
        out["mid"] = (nr // 3, max(nr // 3, 2 * nr // 3))
        out["mid_tracks"] = e.walk_span(w, 2, tracks=True, records=out["mid"])
        out["need2"] = e.hbm_needed()
        out["stats2"] = e.stats()
        out["fin_again"] = e.finish()
        e.reprune(u.coverage + 2)
        out["fin_repruned"] = e.finish()
        out["whole_repruned"] = e.pair_span()
    return out


@pytest.fixture(scope="module")
def engine_of(agx, modelled):
    made = {}

    def get(name):
        if name not in made:
            made[name] = run_engine(agx, modelled(name))
        return made[name]
    return get


def assert_span(got, want, what):
    d = SM.same_span(got, want)
    assert d is None, (what, d, np.asarray(got[d]).tolist()[:20] if not np.isscalar(got[d]) else got[d], np.asarray(want[d]).tolist()[:20] if not np.isscalar(want[d]) else want[d])


def assert_same(got, want, what):
    d = SM.same(got, want, tracks=True)
    assert d is None, (what, d, np.asarray(got[d]).tolist()[:20] if not np.isscalar(got[d]) else got[d], np.asarray(want[d]).tolist()[:20] if not np.isscalar(want[d]) else want[d])


@pytest.mark.parametrize("name", NAMES)
def test_pair_span_windows(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for win, got in e["pair"].items():
        assert_span(got, SM.pair_span(m["front"], win, m["frags"]), win)
    whole = SM.pair_span(m["front"], None, m["frags"])
    assert_span(e["whole"], whole, "whole")
    assert_span(e["again"], whole, "a second call")
    assert int(e["whole"]["cross"][-1]) == 0 and e["whole"]["n_outside"] == 0
    assert e["stats0"]["ms_pair_span"] == 0.0 and e["stats0"]["ms_walk_span"] == 0.0 and e["stats1"]["ms_pair_span"] > 0.0 and e["stats1"]["ms_walk_span"] == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_forced_sub_windows(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for (c, win), got in e["sub"].items():
        assert_span(got, SM.pair_span(m["front"], win, m["frags"]), (c, win))


@pytest.mark.parametrize("name", NAMES)
def test_walk_span_tables(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for k, tab in tables_of(m, e["w"]).items():
        for t in e["ts"][k]:
            assert_same(e["walk"][(k, t)], SM.walk_span(m["front"], m["side_xpos"], tab, t, frags=m["frags"], based=e["based"][k]), (k, t))
    for k in ("rec_len", "st_off", "id_first", "id_last", "base_off", "joined"):      # the serial executor's walk kept the same stretches
        assert np.array_equal(e["w"][k], m["w"][k]), k
    own = e["walk"][("own", 0)]
    assert own["n_steps_not_forward"] == 0 and len(own["iv_rec"]) == 0
    above = e["ts"]["own"][3]
    every = e["walk"][("own", above)]
    assert int((every["iv_last"].astype(np.int64) - every["iv_first"] + 1).sum()) == every["n_graph_bases"]      # above every span every graph base is thin
    want = SM.walk_span(m["front"], m["side_xpos"], e["w"], 2, frags=m["frags"], based=e["based"]["own"])
    for k in SM.TOTALS + SM.REC_KEYS + SM.IV_KEYS:      # w=None takes the unit's own stretches
        assert np.array_equal(np.asarray(e["default"][k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), k
    if "jumps" in m["tables"]:
        j = e["walk"][("jumps", 1)]
        assert j["n_jump_steps"] >= 5 and j["n_steps_not_forward"] >= 2 and j["pos"][63] == 63 and j["pos"][64] == 68
    assert e["stats2"]["ms_walk_span"] > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_forced_base_chunks(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for (c, k, t), got in e["chunks"].items():
        assert_same(got, e["walk"][(k, t)], (c, k, t))


@pytest.mark.parametrize("name", NAMES)
def test_tracks_of_a_middle_record_range(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    assert_same(e["mid_tracks"], SM.walk_span(m["front"], m["side_xpos"], e["w"], 2, records=e["mid"], frags=m["frags"], based=e["based"]["own"]), e["mid"])
    assert (e["mid_tracks"]["rec_lo"], e["mid_tracks"]["rec_hi"]) == e["mid"]


@pytest.mark.parametrize("name", NAMES)
def test_disturbs_nothing(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    assert e["fin_again"] == e["fin"]                                                    # the finish behind it all, byte for byte
    assert e["stats0"]["device_bytes"] == e["stats1"]["device_bytes"] == e["stats2"]["device_bytes"] and e["need"] == e["need2"]      # sampled after one export
    assert_span(e["whole_repruned"], SM.pair_span(m["front"], None, m["frags"]), "after reprune + finish")      # nothing depends on the coverage threshold


def test_unit_without_edge_support_and_paths(agx, modelled):
    m = modelled("walk_kinds")
    with built_unit(agx, m, keep_paths=False) as e:
        before = e.stats()["device_bytes"]
        for k, tab in m["tables"].items():
            assert_same(e.walk_span(tab, 1, tracks=True), SM.walk_span(m["front"], m["side_xpos"], tab, 1, frags=m["frags"]), k)
        assert_span(e.pair_span(), SM.pair_span(m["front"], None, m["frags"]), "no paths")
        with pytest.raises(agx.AgxError) as x:
            e.walk_span()
        assert x.value.code == agx.AGX_E_ARG and "AGX_FLAG_KEEP_PATHS" in x.value.msg      # (walk_paths(): there is no table of its own)
        assert len(m["tables"]) == 2 and e.stats()["device_bytes"] >= before


def test_holds_what_an_export_holds(agx, modelled):
    """The scratch is the export's buffer: a unit that asks holds the bytes the same unit holds after an export."""
    m = modelled("seed203")
    held = []
    for ask in (lambda e: e.unitigs(), lambda e: e.pair_span(), lambda e: e.walk_span(min_span=2, tracks=True)):
        with built_unit(agx, m) as e:
            e.finish()
            ask(e)
            held.append(e.stats()["device_bytes"])
    assert held[0] == held[1] == held[2]


def test_refusals_leave_the_unit_as_it_was(agx, modelled):
    m = modelled("walk_hops")
    hand, n_pos = m["tables"]["hand"], m["n_pos"]

    def refused(call, what, *a, code=None, **kw):
        with pytest.raises(agx.AgxError) as x:
            call(*a, **kw)
        assert x.value.code == (agx.AGX_E_ARG if code is None else code) and what in x.value.msg, x.value.msg

    with built_unit(agx, m) as e:
        fin = e.finish()
        want_w, want_p = e.walk_span(hand, 2), e.pair_span((5, 70))
        before = e.stats()["device_bytes"]
        for what, table in malformed(hand):
            refused(e.walk_span, what, table, 2)
        refused(e.walk_span, "track records", hand, 0, tracks=True, records=(3, 2))
        refused(e.walk_span, "track records", hand, 0, tracks=True, records=(0, len(hand["rec_len"]) + 1))
        refused(e.pair_span, "window", (6, 5))
        refused(e.pair_span, "window", (0, n_pos + 1))
        assert e.stats()["device_bytes"] == before and e.finish() == fin
        assert SM.same(e.walk_span(hand, 2), want_w) is None and SM.same_span(e.pair_span((5, 70)), want_p) is None
        e.download()
        refused(e.pair_span, "not built")                                  # downloaded
        refused(e.walk_span, "not built", hand)
        e.trim()
        refused(e.pair_span, "not built")                                  # trimmed
        refused(e.walk_span, "not built", hand)
        assert e.finish() == fin
    with built_unit(agx, m) as e:
        e.release()
        refused(e.pair_span, "not built")                                  # released
        refused(e.walk_span, "not built", hand)
    with built_unit(agx, m, build=False) as e:
        refused(e.pair_span, "not built")                                  # not built yet
        refused(e.walk_span, "not built", hand)
        e.build()
        assert e.finish() == fin
    with built_unit(agx, m, keep_counts=False, keep_paths=False) as e:
        before = e.stats()["device_bytes"]
        refused(e.pair_span, "AGX_FLAG_KEEP_COUNTS")
        refused(e.walk_span, "AGX_FLAG_KEEP_COUNTS", hand)
        assert e.stats()["device_bytes"] == before and e.finish() == fin
    with built_unit(agx, m, flags=agx.AGX_FLAG_ONE_SHOT) as e:
        refused(e.pair_span, "one-shot")
        refused(e.walk_span, "one-shot", hand)
        assert e.finish() == fin


def test_a_unit_that_never_asks_plans_and_holds_what_it_did(agx, modelled):
    """The feature has no flag and reserves nothing: hbm_needed(), device_bytes and the outputs of a build + finish are the same before any unit of the process has asked
    and after one has; a unit that does not ask reports no span time."""
    m = modelled("seed201")

    def measure(ask):
        with built_unit(agx, m) as e:
            need = e.hbm_needed()
            fin = e.finish()
            e.unitigs()
            if ask:
                e.pair_span()
                e.walk_span(min_span=2, tracks=True)
            st = e.stats()
            assert (st["ms_pair_span"] > 0.0) == ask and (st["ms_walk_span"] > 0.0) == ask
            return need, st["device_bytes"], fin
    before, asked, after = measure(False), measure(True), measure(False)
    assert before == after == asked
