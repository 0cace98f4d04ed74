"""The mate links on the device (agx_links.hip, agx_unit_mate_links) against tests/links_model.py on the units and tables of
tests/test_links_cases.py.  Per unit one build serves every check: every table at min_pairs 0, 1, 2 and one above every count, field by field; w=None; a second call;
slot counts forced through AGX_LINKS_SLOTS on a table of single-base records cut to a power of two of links — exactly that many slots (one pass), half of them (the
records are split and the answer stays, or a record's links alone do not fit and the call is refused with that record) and 2 slots where a record has three links
(refused); the same answer after reprune + finish; a unit without edge counters and kept paths; the refusals of span_check and check_walk_table; and that the call plans
and holds what an export does, reports its own time and leaves the finish's bytes alone.  Past one grid of hit records: the G + 257 unit of
tests/span_wide_units.py with records under the highest first tile, so that links come from hit records behind G in the device's order.  Every comparison is integer
equality."""
import os

import numpy as np
import pytest

import links_model as LM
import links_units as LU
import path_model as PM
import span_wide as SW
import span_wide_units as WU
from test_gpu_evidence import malformed
from test_links_cases import UNITS, modelled, tables_of, thresholds  # noqa: F401  (modelled: the module fixture)

pytestmark = pytest.mark.gpu

NAMES = list(UNITS)


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


def forced(slots, call, *a, **kw):
    os.environ["AGX_LINKS_SLOTS"] = str(slots)
    try:
        return call(*a, **kw)
    finally:
        del os.environ["AGX_LINKS_SLOTS"]


def cut_table(m):
    """(table of single-base records over positions [0, R), K): the R for which the table has exactly K = the largest power of two of links that some R gives, K >= 4;
    (None, 0) if no R does.  Record x is position x, so the links are the distinct fragments (f_lo, f_hi) with f_lo < f_hi < R."""
    f = np.unique(np.stack([m["frags"][0], m["frags"][1]], 1), axis=0) if len(m["frags"][0]) else np.zeros((0, 2), np.int64)
    f = f[(f[:, 0] < f[:, 1]) & (f[:, 1] < LU.EVERY_BASE_MAX)]
    best = (None, 0)
    for r in np.unique(f[:, 1]).tolist():
        k = int((f[:, 1] <= r).sum())
        if k >= 4 and k & (k - 1) == 0 and k > best[1]:
            best = (PM.stretches([(1, [(x, x, 0, 0)]) for x in range(r + 1)]), k)
    return best


def run_engine(agx, m):
    """One build of the unit; everything the tests look at, collected before the unit goes."""
    u, out = m["u"], {}
    with built_unit(agx, m) as e:
        out["need"] = e.hbm_needed()
        out["fin"] = e.finish()
        w = out["w"] = e.walk_paths()
        e.unitigs()
        out["stats0"] = e.stats()
        tabs = out["tables"] = dict(tables_of(m), own=w)
        model = lambda tab, t: LM.mate_links(m["frags"], m["n_pos"], m["side_xpos"], tab, t)
        out["ts"] = {k: thresholds(model(tab, 1)) for k, tab in tabs.items()}
        out["links"] = {(k, t): e.mate_links(tab, t) for k, tab in tabs.items() for t in out["ts"][k]}
        out["default"] = e.mate_links()
        out["again"] = e.mate_links(tabs["every_base"], 1)
        out["stats1"] = e.stats()
        cut, k = out["cut"] = cut_table(m)
        if cut is not None:
            out["cut_want"] = model(cut, 1)
            out["cut_exact"] = forced(k, e.mate_links, cut, 1)
            try:
                out["cut_half"] = forced(k // 2, e.mate_links, cut, 2)
            except agx.AgxError as x:
                out["cut_half"] = x
        try:
            out["two"] = forced(2, e.mate_links, tabs["every_base"], 1)
        except agx.AgxError as x:
            out["two"] = x
        out["after_refusal"] = e.mate_links(tabs["every_base"], 1)
        out["need2"] = e.hbm_needed()
        out["stats2"] = e.stats()
        out["fin_again"] = e.finish()
        e.reprune(u.coverage + 2)
        out["fin_repruned"] = e.finish()
        out["repruned"] = e.mate_links(tabs["interleaved"], 1)
    return out


@pytest.fixture(scope="module")
def engine_of(agx, modelled):
    made = {}

    def get(name):
        if name not in made:
            made[name] = run_engine(agx, modelled(name))
        return made[name]
    return get


def assert_same(got, want, what):
    d = LM.same(got, want)
    assert d is None, (what, d, np.asarray(got[d]).tolist()[:20] if not np.isscalar(got[d]) else got[d], np.asarray(want[d]).tolist()[:20] if not np.isscalar(want[d]) else want[d])
    assert LM.identity(got), what


def wanted(m, tab, t):
    return LM.mate_links(m["frags"], m["n_pos"], m["side_xpos"], tab, t)


@pytest.mark.parametrize("name", NAMES)
def test_tables_and_thresholds(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for (k, t), got in e["links"].items():
        assert_same(got, wanted(m, e["tables"][k], t), (k, t))
        assert got["n_passes"] == 1 and got["n_slots"] >= 2 and got["n_slots"] & (got["n_slots"] - 1) == 0
    for k in ("rec_len", "st_off", "id_first", "id_last", "base_off", "joined"):      # the serial executor's walk kept the same stretches
        assert np.array_equal(e["w"][k], m["w"][k]), k
    assert_same(e["default"], wanted(m, e["w"], 1), "w=None")
    assert_same(e["again"], wanted(m, e["tables"]["every_base"], 1), "a second call")
    assert_same(e["after_refusal"], wanted(m, e["tables"]["every_base"], 1), "after a refused call")
    assert e["links"][("one_record", 1)]["n_links_all"] == 0 and e["links"][("empty", 1)]["n_owned"] == 0
    assert all(got["ms"] > 0.0 for got in e["links"].values()) and "ms_mate_links" not in e["stats1"]      # the time is the call's own; agx_stats is as it was


@pytest.mark.parametrize("name", NAMES)
def test_forced_slot_counts(agx, engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    cut, k = e["cut"]
    if cut is not None:
        assert e["cut_want"]["n_links_all"] == k
        assert_same(e["cut_exact"], e["cut_want"], ("exactly", k))
        assert e["cut_exact"]["n_passes"] == 1 and e["cut_exact"]["n_slots"] == k                 # every key still finds a slot in one pass
        out = np.bincount(e["cut_want"]["a"], minlength=len(cut["rec_len"]))
        if isinstance(e["cut_half"], dict):
            assert_same(e["cut_half"], wanted(m, cut, 2), ("half", k // 2))
            assert e["cut_half"]["n_passes"] >= 3 and e["cut_half"]["n_slots"] == k // 2 and out.max() <= k // 2      # the range was split and the answer stayed
        else:
            assert e["cut_half"].code == agx.AGX_E_UNSUPPORTED and out.max() > k // 2, e["cut_half"].msg
    out = np.bincount(wanted(m, e["tables"]["every_base"], 1)["a"], minlength=1)
    if out.max() >= 3:
        assert not isinstance(e["two"], dict) and e["two"].code == agx.AGX_E_UNSUPPORTED and "record %d alone" % int(np.nonzero(out >= 3)[0][0]) in e["two"].msg, e["two"]
    elif isinstance(e["two"], dict):
        assert_same(e["two"], wanted(m, e["tables"]["every_base"], 1), "2 slots")


def test_forced_slot_counts_reach_their_shapes(agx, engine_of, modelled):
    """Among the units: a table cut to K links that K slots hold in one pass, one that K / 2 slots hold after a split, and the refusal at 2 slots."""
    seen = set()
    for name in NAMES:
        e = engine_of(name)
        if e["cut"][0] is not None:
            seen.add("exact")
            if isinstance(e["cut_half"], dict):
                seen.add("split")
        if not isinstance(e["two"], dict):
            seen.add("refused")
    assert seen == {"exact", "split", "refused"}, seen


@pytest.mark.parametrize("name", NAMES)
def test_disturbs_nothing(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    assert e["fin_again"] == e["fin"]                                                    # the finish behind it all, byte for byte
    assert e["stats0"]["device_bytes"] == e["stats1"]["device_bytes"] == e["stats2"]["device_bytes"] and e["need"] == e["need2"]      # sampled after one export
    assert_same(e["repruned"], wanted(m, e["tables"]["interleaved"], 1), "after reprune + finish")      # nothing depends on the coverage threshold


def test_bad_slot_counts_are_refused(agx, modelled):
    m = modelled("walk_kinds")
    tab = LU.links_tables(m["n_pos"])["interleaved"]
    with built_unit(agx, m) as e:
        fin = e.finish()
        for bad in ("0", "1", "3", "6", "-4", "8x", "", str(1 << 32)):
            with pytest.raises(agx.AgxError) as x:
                forced(bad, e.mate_links, tab, 1)
            assert x.value.code == agx.AGX_E_ARG and "AGX_LINKS_SLOTS" in x.value.msg, (bad, x.value.msg)
        assert_same(forced(4, e.mate_links, tab, 1), wanted(m, tab, 1), "4 slots")
        assert e.finish() == fin


def test_unit_without_edge_support_and_paths(agx, modelled):
    m = modelled("walk_kinds")
    with built_unit(agx, m, keep_paths=False) as e:
        before = e.stats()["device_bytes"]
        for k, tab in tables_of(m).items():
            assert_same(e.mate_links(tab, 1), wanted(m, tab, 1), k)
        with pytest.raises(agx.AgxError) as x:
            e.mate_links()
        assert x.value.code == agx.AGX_E_ARG and "AGX_FLAG_KEEP_PATHS" in x.value.msg      # (walk_paths(): there is no table of its own)
        assert e.stats()["device_bytes"] >= before


def test_refusals_leave_the_unit_as_it_was(agx, modelled):
    m = modelled("walk_hops")
    hand = m["tables"]["hand"]

    def refused(call, what, *a, code=None, **kw):
        with pytest.raises(agx.AgxError) as x:
            call(*a, **kw)
        assert x.value.code == (agx.AGX_E_ARG if code is None else code) and what in x.value.msg and x.value.msg.startswith("mate links"), x.value.msg

    with built_unit(agx, m) as e:
        fin = e.finish()
        want = e.mate_links(hand, 2)
        before = e.stats()["device_bytes"]
        for what, table in malformed(hand):
            refused(e.mate_links, what, table, 2)
        assert e.stats()["device_bytes"] == before and e.finish() == fin
        assert LM.same(e.mate_links(hand, 2), want) is None
        e.download()
        refused(e.mate_links, "not built", hand)                                  # downloaded
        e.trim()
        refused(e.mate_links, "not built", hand)                                  # trimmed
        assert e.finish() == fin
    with built_unit(agx, m) as e:
        e.release()
        refused(e.mate_links, "not built", hand)                                  # released
    with built_unit(agx, m, build=False) as e:
        refused(e.mate_links, "not built", hand)                                  # not built yet
        e.build()
        assert e.finish() == fin
    with built_unit(agx, m, keep_counts=False, keep_paths=False) as e:
        before = e.stats()["device_bytes"]
        refused(e.mate_links, "AGX_FLAG_KEEP_COUNTS", hand)
        assert e.stats()["device_bytes"] == before and e.finish() == fin
    with built_unit(agx, m, flags=agx.AGX_FLAG_ONE_SHOT) as e:
        refused(e.mate_links, "one-shot", hand)
        assert e.finish() == fin


def test_a_unit_that_never_asks_plans_and_holds_what_it_did(agx, modelled):
    """The feature has no flag and reserves nothing: hbm_needed(), device_bytes and the outputs of a build + finish are the same before any unit of the process has asked
    and after one has; a unit that asks holds what the same unit holds after an export."""
    m = modelled("seed201")

    def measure(ask):
        with built_unit(agx, m) as e:
            need = e.hbm_needed()
            fin = e.finish()
            e.unitigs()
            if ask:
                e.mate_links(min_pairs=2)
            st = e.stats()
            return need, st["device_bytes"], fin
    before, asked, after = measure(False), measure(True), measure(False)
    assert before == after == asked
    with built_unit(agx, m) as e:
        e.finish()
        e.mate_links()
        assert e.stats()["device_bytes"] == asked[1]


# ---- past one grid of hit records ------------------------------------------------------------------------------------------------

def wide_table():
    """Records under the highest first tile — four of twelve positions each, a gap of four behind every one — behind a record over the 400 positions in front of the tile:
    the fragments of the hit records behind G begin in that tile, so their left ends lie under these records (or in the gaps)."""
    top = WU.TOP_TILE * WU.TILE
    recs = [(400, [(top - 400, top - 1, 0, 0)])] + [(12, [(top + 16 * i, top + 16 * i + 11, 0, 0)]) for i in range(4)] + [(WU.N_POS - top - 64, [(top + 64, WU.N_POS - 1, 0, 0)])]
    return PM.stretches(recs)


def test_past_one_grid_of_hits(agx, built, tmp_path_factory):
    g, sh = WU.grid_hits(), WU.shapes()
    n_hits = WU.CASES["G+257"](g)
    full = WU.write_full(str(tmp_path_factory.mktemp("links_wide_full")), g, sh)
    tmp = WU.write_case(full, str(tmp_path_factory.mktemp("links_wide")), n_hits, sh)
    w = wide_table()
    with agx.Unit(k=WU.K, insert_variation=WU.IV, coverage=WU.COVERAGE, keep_counts=True, keep_paths=True) as e:
        e.load_files(tmp, 0)
        e.upload()
        e.build()
        front = e.front()
        fin = e.finish()
        got = {t: e.mate_links(w, t) for t in (1, 2)}
        split = forced(8, e.mate_links, w, 1)
        assert e.finish() == fin
    assert front["n_hits"] == n_hits == g + 257
    f_lo, f_hi, at, kept, outside = SW.fragments_at(front)
    frags = (f_lo, f_hi, int(kept.sum()), int(outside.sum()))
    side = np.zeros(0, np.uint32)      # (the table holds main ids only)
    for t in (1, 2):
        assert_same(got[t], LM.mate_links(frags, WU.N_POS, side, w, t), ("wide", t))
    want = LM.mate_links(frags, WU.N_POS, side, w, 1)
    assert_same(split, want, "wide, 8 slots")
    # links that only the records behind G make: without them the table is another
    early = at < g
    less = LM.mate_links((f_lo[early], f_hi[early], int(early.sum()), 0), WU.N_POS, side, w, 1)
    assert int((~early).sum()) > 0 and want["n_link_pairs"] > less["n_link_pairs"] and want["n_links_all"] >= 2
