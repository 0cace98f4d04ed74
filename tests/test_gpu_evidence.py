"""Evidence under the walk's records on the device (agx_k_ev_gather, agx_k_ev_runs, agx_unit_walk_evidence) against tests/evidence_model.py on the
units of tests/test_evidence_cases.py: every case of tests/walk_units.py and the generated seeds 201 and 203.  Per unit one build serves every check: the stretches of its
own finish and the hand-made stretch tables (test_evidence_cases.hand_made: a stretch across the 64-base wave border, one-base stretches, records inside one wave with
equal minima, joined and unjoined boundaries, side ids, ids without a node, a pair without an edge, steps out of nodes with overflow edges) at several (min_depth,
min_support) pairs, whole table and field by field; the same answers in chunks of 64 and 128 bases; tracks of a middle record range; the answer after a reprune and
another finish; a unit without edge counters; the refusals; and that a unit which never asks plans and holds what it did."""
import os

import numpy as np
import pytest

import evidence_model as EM
import path_model as PM
import walk_model as WM
from test_evidence_cases import SEED_UNITS, UNITS, WALK_UNITS, hand_made, modelled, thresholds  # noqa: F401  (modelled: the module fixture)

pytestmark = pytest.mark.gpu

NAMES = [u.name for u in WALK_UNITS + SEED_UNITS]
NONE = EM.NONE


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def built_unit(agx, m, **kw):
    u = m["u"]
    flags = dict(keep_counts=True, keep_paths=True, edge_support=True)
    flags.update(kw)
    e = agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, **flags)
    e.load_files(m["tmp"], 0)
    e.upload()
    e.build()
    return e


def chunked(e, chunk, *a, **kw):
    os.environ["AGX_EVIDENCE_CHUNK"] = str(chunk)
    try:
        return e.walk_evidence(*a, **kw)
    finally:
        del os.environ["AGX_EVIDENCE_CHUNK"]


def run_engine(agx, m):
    """One build of the unit; everything the tests look at, collected before the unit goes."""
    u, g = m["u"], m["g"]
    out = {}
    with built_unit(agx, m) as e:
        out["fin"] = e.finish()
        w = out["w"] = e.walk_paths()
        out["stats0"] = e.stats()
        out["own"] = {t: e.walk_evidence(w, t[0], t[1], tracks=True) for t in thresholds(g, u.coverage)}
        out["stats1"] = e.stats()
        out["default"] = e.walk_evidence(min_depth=u.coverage, min_support=2)
        out["hand"] = {t: e.walk_evidence(m["hand"], t[0], t[1], tracks=True) for t in thresholds(g, u.coverage)}
        above = thresholds(g, u.coverage)[2]
        out["chunks"] = {(c, t): chunked(e, c, tab, t[0], t[1], tracks=True) for c in (64, 128) for t in ((u.coverage, 2), above) for tab in (m["hand"],)}
        out["own_chunks"] = {c: chunked(e, c, w, above[0], above[1], tracks=True) for c in (64, 128)}
        nr = len(w["rec_len"])
        out["mid"] = (nr // 3, max(nr // 3, 2 * nr // 3))
        out["mid_tracks"] = e.walk_evidence(w, u.coverage, 2, tracks=True, records=out["mid"])
        out["hand_mid"] = e.walk_evidence(m["hand"], u.coverage, 2, tracks=True, records=(1, 6))
        out["stats2"] = e.stats()
        out["fin_again"] = e.finish()
        e.reprune(u.coverage + 2)
        out["fin_repruned"] = e.finish()
        out["w_repruned"] = e.walk_paths()
        out["repruned"] = e.walk_evidence(out["w_repruned"], u.coverage + 2, 2, tracks=True)
    return out


@pytest.fixture(scope="module")
def engine_of(agx, modelled):
    made = {}

    def get(name):
        if name not in made:
            made[name] = run_engine(agx, modelled(name))
        return made[name]
    return get


def model(m, w, t, records=None, coverage=None, wm=None, node=None):
    cov = m["u"].coverage if coverage is None else coverage
    return EM.evidence(m["g"], cov, w, m["sup"], t[0], t[1], records=records, wm=m["wm"] if coverage is None else wm, node=m["node"] if coverage is None else node)


def assert_same(got, want, what):
    d = EM.same(got, want, tracks=True)
    assert d is None, (what, d, np.asarray(got[d]).tolist()[:20] if d in got and not np.isscalar(got[d]) else got.get(d), np.asarray(want[d]).tolist()[:20] if not np.isscalar(want[d]) else want[d])


@pytest.mark.parametrize("name", NAMES)
def test_stretches_of_the_finish(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    assert e["fin"]["pre"] == m["pre"]
    for k in ("rec_len", "st_off", "id_first", "id_last", "base_off", "joined"):      # the serial executor's walk kept the same stretches
        assert np.array_equal(e["w"][k], m["w"][k]), k
    for t, got in e["own"].items():
        assert_same(got, model(m, e["w"], t), t)
        assert got["n_steps_without_edge"] == 0
    assert len(e["own"][(0, 0)]["iv_rec"]) == 0 and (e["own"][(0, 0)]["depth"] != NONE).all()      # the walk only stands on nodes
    above = thresholds(m["g"], m["u"].coverage)[2]
    every = e["own"][above]
    assert int((every["iv_last"].astype(np.int64) - every["iv_first"] + 1).sum()) == every["n_graph_bases"] > 0      # above every depth every graph base is weak
    want = model(m, e["w"], (m["u"].coverage, 2))
    for k in EM.TOTALS + EM.REC_KEYS + EM.IV_KEYS:      # w=None takes the unit's own stretches
        assert np.array_equal(np.asarray(e["default"][k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), k
    assert e["stats0"]["ms_walk_evidence"] == 0.0 and e["stats1"]["ms_walk_evidence"] > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_hand_made_stretches(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for t, got in e["hand"].items():
        assert_same(got, model(m, m["hand"], t), t)
    got = e["hand"][(0, 0)]
    assert got["n_steps_without_edge"] >= 1                  # the backwards pair
    assert got["rec_depth_min_at"][5] == 0                   # two offsets of record 5 share its smallest depth: the smaller one
    assert_same(e["hand_mid"], model(m, m["hand"], (m["u"].coverage, 2), records=(1, 6)), "records 1 .. 6")


@pytest.mark.parametrize("name", NAMES)
def test_chunks_give_the_unchunked_answer(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    for (c, t), got in e["chunks"].items():
        assert_same(got, e["hand"][t], (c, t))
    above = thresholds(m["g"], m["u"].coverage)[2]
    whole = e["hand"][above]
    pre = np.concatenate(([0], np.cumsum(m["hand"]["id_last"].astype(np.int64) - m["hand"]["id_first"] + 1)))
    # an interval of the unchunked answer lies across flat base 64: record 1's stretch, every base weak
    s1 = int(m["hand"]["st_off"][1])
    assert pre[s1] < 64 < pre[s1 + 1] and ((whole["iv_rec"] == 1) & (whole["iv_first"] == 0) & (whole["iv_last"] == pre[s1 + 1] - pre[s1] - 1)).any()
    for c, got in e["own_chunks"].items():
        assert_same(got, e["own"][above], c)


@pytest.mark.parametrize("name", NAMES)
def test_tracks_of_a_middle_record_range(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    assert_same(e["mid_tracks"], model(m, e["w"], (m["u"].coverage, 2), records=e["mid"]), e["mid"])
    assert (e["mid_tracks"]["rec_lo"], e["mid_tracks"]["rec_hi"]) == e["mid"]


@pytest.mark.parametrize("name", NAMES)
def test_after_reprune_and_finish(engine_of, modelled, name):
    m, e = modelled(name), engine_of(name)
    cov = m["u"].coverage + 2
    wm = WM.build(m["g"], cov)
    node = PM.id_nodes(m["g"], cov, wm)
    assert_same(e["repruned"], model(m, e["w_repruned"], (cov, 2), coverage=cov, wm=wm, node=node), "repruned")
    assert e["repruned"]["n_steps_without_edge"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_disturbs_nothing(engine_of, name):
    e = engine_of(name)
    assert e["fin_again"] == e["fin"]
    assert e["stats1"]["device_bytes"] == e["stats2"]["device_bytes"]      # whatever is asked and however often, the calls share one buffer: the export's
    if e["stats0"]["build_attempts"] == 1:      # (a unit whose pool grew has left the block that reserved the export's scratch: its first export of any kind takes it anew)
        assert e["stats0"]["device_bytes"] == e["stats2"]["device_bytes"], e["stats0"]["build_attempts"]


@pytest.mark.parametrize("name", ["seed203", "walk_kinds"])
def test_holds_what_an_export_holds(agx, modelled, name):
    """The scratch is the export's buffer: a unit that asks for evidence holds the bytes the same unit holds after an export, also where the pool grew."""
    m = modelled(name)
    held = []
    for ask in (lambda e: e.unitigs(), lambda e: e.walk_evidence(min_depth=m["u"].coverage, min_support=2, tracks=True)):
        with built_unit(agx, m) as e:
            e.finish()
            ask(e)
            held.append(e.stats()["device_bytes"])
    assert held[0] == held[1]


def test_unit_without_edge_support(agx, modelled):
    m = modelled("walk_kinds")
    u = m["u"]
    with built_unit(agx, m, edge_support=False, keep_paths=False) as e:      # (keep_paths is not needed: the table is the caller's)
        before = e.stats()["device_bytes"]
        got = e.walk_evidence(m["hand"], u.coverage, 0, tracks=True)
        assert_same(got, EM.evidence(m["g"], u.coverage, m["hand"], None, u.coverage, 0, wm=m["wm"], node=m["node"]), "no counters")
        assert (got["step"] == NONE).all() and got["n_steps"] == 0
        with pytest.raises(agx.AgxError) as x:
            e.walk_evidence(m["hand"], 0, 1)
        assert x.value.code == agx.AGX_E_ARG and "AGX_FLAG_EDGE_SUPPORT" in x.value.msg
        assert e.stats()["device_bytes"] == before


def malformed(w):
    """(what the message names, table): one rule of the host's checks broken each"""
    def mut(**kw):
        t = {k: np.array(v, copy=True) for k, v in w.items()}
        for k, (i, v) in kw.items():
            t[k][i] = v
        return t
    s = int(w["st_off"][6])          # record 6: (a, a + 1, 0, 0), (a + 2, a + 3, 2, 1), (a + 4, a + 4, 4, 0)
    return [("st_off", mut(st_off=(0, 1))), ("monotone", mut(st_off=(3, int(w["st_off"][4]) + 1))),
            ("inside its record", mut(rec_len=(1, 3))), ("overlaps", mut(base_off=(s + 1, 1))), ("id_last < id_first", mut(id_last=(s + 1, int(w["id_first"][s + 1]) - 1))),
            ("not a walk id", mut(id_last=(0, 0xFFFFFFF0))), ("joined", mut(joined=(s, 1))), ("joined", mut(joined=(s + 2, 1), base_off=(s + 2, 5))),
            ("joined is neither", mut(joined=(s + 1, 2)))]


def test_refusals_leave_the_unit_as_it_was(agx, modelled):
    m = modelled("walk_hops")
    u, hand = m["u"], m["hand"]

    def refused(e, what, *a, code=None, **kw):
        with pytest.raises(agx.AgxError) as x:
            e.walk_evidence(*a, **kw)
        assert x.value.code == (agx.AGX_E_ARG if code is None else code) and what in x.value.msg, x.value.msg

    with built_unit(agx, m) as e:
        fin = e.finish()
        want = e.walk_evidence(hand, u.coverage, 2)
        before = e.stats()["device_bytes"]
        for what, table in malformed(hand):
            refused(e, what, table, u.coverage, 2)
        refused(e, "track records", hand, 0, 0, tracks=True, records=(3, 2))
        refused(e, "track records", hand, 0, 0, tracks=True, records=(0, len(hand["rec_len"]) + 1))
        assert e.stats()["device_bytes"] == before and e.finish() == fin
        assert EM.same(e.walk_evidence(hand, u.coverage, 2), want) is None
        e.download()
        e.trim()
        refused(e, "not built", hand)
        assert e.finish() == fin
    with built_unit(agx, m, keep_counts=False) as e:
        before = e.stats()["device_bytes"]
        refused(e, "AGX_FLAG_KEEP_COUNTS", hand)
        assert e.stats()["device_bytes"] == before and e.finish() == fin
    with built_unit(agx, m, edge_support=False, flags=agx.AGX_FLAG_ONE_SHOT) as e:
        assert EM.same(e.walk_evidence(hand, u.coverage, 0), EM.evidence(m["g"], u.coverage, hand, None, u.coverage, 0, wm=m["wm"], node=m["node"])) is None      # before its download
        assert e.finish() == fin
        refused(e, "one-shot", hand)
    with built_unit(agx, m, flags=agx.AGX_FLAG_ONE_SHOT) as e:               # the counting's own check: it reads the front of the build
        refused(e, "one-shot", hand)
        assert e.finish() == fin


def test_a_unit_that_never_asks_plans_and_holds_what_it_did(agx, modelled):
    """The feature has no flag and reserves nothing: hbm_needed(), device_bytes and the outputs of a build + finish are the same before any unit of the process has asked
    and after one has; a unit that does not ask reports no evidence time."""
    m = modelled("seed201")

    def measure(ask):
        with built_unit(agx, m) as e:
            need = e.hbm_needed()
            fin = e.finish()
            if ask:
                e.walk_evidence(min_depth=m["u"].coverage, min_support=2, tracks=True)
            st = e.stats()
            assert (st["ms_walk_evidence"] > 0.0) == ask
            return need, st["device_bytes"], fin
    before, asked, after = measure(False), measure(True), measure(False)
    assert before == after == asked
