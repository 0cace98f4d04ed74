"""Edge support on the device (agx_k_edge_support, agx_unit_edge_support, agx_unit_unitigs_support) against tests/edge_support_model.py on the
units of tests/test_edge_support_cases.py: every case of tests/edge_units.py and the generated seeds 201 and 203.  Per unit one build serves every check: the counts in
agx_unit_graph's numbering, a second call, the counts after a reprune, the links' support of the whole unit, of a middle window and at a threshold below and above the
build's, and the tagged GFA text.  The overflow cases also run with every capacity starting small (the counters follow a regrown pool and list), the cases with edges across
window cuts with the upload cut in two."""
import os
import re

import numpy as np
import pytest

import edge_support_model as ESM
from gpu_checks import check_counts
from test_edge_support_cases import EDGE_UNITS, SEED_UNITS, UNITS, modelled  # noqa: F401  (modelled: the module fixture)

pytestmark = pytest.mark.gpu

NAMES = [u.name for u in EDGE_UNITS + SEED_UNITS]
NONE = ESM.NONE
MAXE = 4
UNITIG_KEYS = ("head_pos", "head_var", "n_nodes", "last_pos", "coverage", "seq_off", "seq", "link_from", "link_to")


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def exports(u_, n_pos, cov):
    """(label, region, min_coverage) of the exports every unit is asked for: the whole unit, a middle window, a threshold below and one above the build's"""
    mid = (n_pos // 3 // 64 * 64 + 7, min(n_pos, 2 * n_pos // 3 + 13))
    return [("whole", None, None), ("middle", mid, None), ("below", None, 0), ("above", None, cov + 3)]


def run_engine(agx, u, tmp, reprune_to=None):
    """One build of the unit with the flag; everything the tests look at, collected before the unit goes."""
    out = {}
    with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, keep_counts=True, edge_support=True) as e:
        e.load_files(tmp, 0)
        e.upload()
        e.build()
        out["stats0"] = e.stats()
        out["first"] = e.edge_support()
        out["stats1"] = e.stats()
        out["second"] = e.edge_support()
        out["stats2"] = e.stats()
        out["graph"] = e.graph()
        n_pos = out["graph"]["n_pos"]
        out["exports"] = {}
        for label, region, cov in exports(u, n_pos, u.coverage):
            out["exports"][label] = (region, cov, e.unitigs(region=region, min_coverage=cov, edge_support=True),
                                     e.unitigs(region=region if region is not None else (0, n_pos), min_coverage=cov))
        out["gfa"], out["gfa_tagged"] = e.gfa(3), e.gfa(3, edge_support=True)
        out["stats3"] = e.stats()
        if reprune_to is not None:
            e.reprune(reprune_to)
            out["repruned"] = e.edge_support()
            out["repruned_links"] = e.unitigs(min_coverage=u.coverage, edge_support=True)
    return out


@pytest.fixture(scope="module")
def engine_of(agx, modelled):
    made = {}

    def get(name):
        if name not in made:
            u, tmp, g, front, model = modelled(name)
            made[name] = run_engine(agx, u, tmp, reprune_to=u.coverage + 2)
        return made[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_counts_match_model(engine_of, modelled, name):
    u, tmp, g, front, model = modelled(name)
    e = engine_of(name)
    check_counts(e["first"], e["graph"], model)
    assert e["stats1"]["n_support_events"] == model["n_events"] and e["stats0"]["n_support_events"] == 0
    assert e["stats0"]["ms_edge_support"] == 0.0 and e["stats1"]["ms_edge_support"] > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_second_call_reuses_the_counters(engine_of, modelled, name):
    e = engine_of(name)
    for k in ("edge_start", "edge_dst", "edge_cnt"):
        assert np.array_equal(e["first"][k], e["second"][k]), k
    assert (e["first"]["n_events"], e["first"]["n_contributions"]) == (e["second"]["n_events"], e["second"]["n_contributions"])
    # a sanity check, not a timing claim: the second call zeroes nothing, launches nothing and waits for nothing
    assert e["stats2"]["ms_edge_support"] <= e["stats1"]["ms_edge_support"]


@pytest.mark.parametrize("name", NAMES)
def test_reprune_leaves_the_counts(engine_of, modelled, name):
    u, tmp, g, front, model = modelled(name)
    e = engine_of(name)
    check_counts(e["repruned"], e["graph"], model)
    region, cov, with_sup, plain = e["exports"]["whole"]
    for k in UNITIG_KEYS + ("link_support",):      # the export at the build's threshold, asked for by number after the reprune
        assert np.array_equal(e["repruned_links"][k], with_sup[k]), k


def tails_of(g, t, lo, hi, cov):
    """The last node of every segment of an export over positions [lo, hi) at threshold cov: from the head along the only alive successor that has no other alive
    predecessor, n_nodes - 1 times."""
    ns = g["node_start"].astype(np.int64)
    nn = int(g["n_nodes"])
    pos = np.repeat(np.arange(int(g["n_pos"])), np.diff(ns))
    alive = ((g["node_key"][:, 0] != NONE) | (g["node_cnt"][:, 0].astype(np.int64) >= cov)) & (pos >= lo) & (pos < hi)
    es = g["edge_start"].astype(np.int64)
    src = np.repeat(np.arange(nn), np.diff(es))
    dst = g["edge_dst"].astype(np.int64)
    keep = alive[src] & alive[dst]
    code = np.unique(src[keep] * (nn + 1) + dst[keep])
    src, dst = code // (nn + 1), code % (nn + 1)
    outdeg, indeg = np.bincount(src, minlength=nn), np.bincount(dst, minlength=nn)
    only = np.full(nn, -1, np.int64)
    only[src] = dst                      # (meaningful where outdeg == 1)
    tails = []
    for hp, hv, n in zip(t["head_pos"].tolist(), t["head_var"].tolist(), t["n_nodes"].tolist()):
        cur = int(ns[hp]) + hv
        assert alive[cur]
        for _ in range(n - 1):
            nxt = int(only[cur])
            assert outdeg[cur] == 1 and indeg[nxt] == 1
            cur = nxt
        assert not (outdeg[cur] == 1 and indeg[only[cur]] == 1), "the segment goes on behind its last node"
        tails.append(cur)
    return np.array(tails, np.int64)


@pytest.mark.parametrize("label", ["whole", "middle", "below", "above"])
@pytest.mark.parametrize("name", NAMES)
def test_link_support_is_the_edge_support(engine_of, modelled, name, label):
    u, tmp, g, front, model = modelled(name)
    e = engine_of(name)
    region, cov, t, plain = e["exports"][label]
    for k in UNITIG_KEYS:      # the table itself is the export's without support
        assert np.array_equal(t[k], plain[k]) if k != "seq" else t[k] == plain[k], k
    lo, hi = region if region is not None else (0, int(g["n_pos"]))
    tails = tails_of(g, t, lo, hi, u.coverage if cov is None else cov)
    ns = g["node_start"].astype(np.int64)
    heads = ns[t["head_pos"].astype(np.int64)] + t["head_var"].astype(np.int64)
    want = [ESM.edge_support_of(model, int(tails[a]), int(heads[b])) for a, b in zip(t["link_from"].tolist(), t["link_to"].tolist())]
    assert None not in want
    assert t["link_support"].tolist() == want


@pytest.mark.parametrize("name", NAMES)
def test_gfa_minus_the_tags_is_the_plain_text(engine_of, name):
    e = engine_of(name)
    assert re.sub(rb"\tRC:i:\d+\n", b"\n", e["gfa_tagged"]) == e["gfa"]
    tags = [int(m) for m in re.findall(rb"^L\t.*\tRC:i:(\d+)$", e["gfa_tagged"], re.M)]
    assert tags == e["exports"]["whole"][2]["link_support"].tolist()


@pytest.mark.parametrize("name", [n for n in NAMES if UNITS[n].overflow])
def test_overflow_case_small_caps(agx, modelled, name, monkeypatch):
    u, tmp, g, front, model = modelled(name)
    monkeypatch.setenv("AGX_TEST_SMALL_CAPS", "1")
    e = run_engine(agx, u, tmp)
    assert e["stats1"]["build_attempts"] > 1 and e["stats1"]["n_edge_overflow"] > 4
    check_counts(e["first"], e["graph"], model)
    region, cov, t, plain = e["exports"]["whole"]
    tails = tails_of(g, t, 0, int(g["n_pos"]), u.coverage)
    heads = g["node_start"].astype(np.int64)[t["head_pos"].astype(np.int64)] + t["head_var"].astype(np.int64)
    assert t["link_support"].tolist() == [ESM.edge_support_of(model, int(tails[a]), int(heads[b])) for a, b in zip(t["link_from"].tolist(), t["link_to"].tolist())]


@pytest.mark.parametrize("name", [n for n in NAMES if UNITS[n].windows])
def test_window_case_upload_in_two_windows(agx, modelled, name, monkeypatch):
    u, tmp, g, front, model = modelled(name)
    monkeypatch.setenv("AGX_UPLOAD_WINDOWS", "2")
    e = run_engine(agx, u, tmp)
    check_counts(e["first"], e["graph"], model)


def test_refusals(agx, modelled):
    u, tmp, g, front, model = modelled("edge_jump")

    def unit(**kw):
        e = agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, **kw)
        e.load_files(tmp, 0)
        e.upload()
        e.build()
        return e

    def refused(e, what):
        for call in (e.edge_support, lambda: e.unitigs(edge_support=True), lambda: e.gfa(edge_support=True)):
            with pytest.raises(agx.AgxError) as x:
                call()
            assert x.value.code == agx.AGX_E_ARG and what in x.value.msg, x.value.msg
    with unit(keep_counts=True) as e:                                  # no flag
        before = e.stats()
        refused(e, "AGX_FLAG_EDGE_SUPPORT")
        after = e.stats()
        assert before["device_bytes"] == after["device_bytes"] and after["n_support_events"] == 0
        assert e.gfa(0)                                                # the unit is as it was
    with unit(keep_counts=True, edge_support=True) as e:               # after download(), then trimmed
        want = e.edge_support()
        e.download()
        refused(e, "not built")
        e.trim()
        refused(e, "not built")
        e.upload()
        e.build()
        assert np.array_equal(e.edge_support()["edge_cnt"], want["edge_cnt"])      # counted again after the new build
    with unit(keep_counts=True, edge_support=True, flags=agx.AGX_FLAG_ONE_SHOT) as e:
        refused(e, "one-shot")
    with unit(edge_support=True) as e:                                 # the counts alone need no kept node counts; the export does
        assert np.array_equal(e.edge_support()["edge_cnt"], model["edge_cnt"])
        with pytest.raises(agx.AgxError) as x:
            e.unitigs(edge_support=True)
        assert x.value.code == agx.AGX_E_ARG and "AGX_FLAG_KEEP_COUNTS" in x.value.msg
    with unit(keep_counts=True, edge_support=True) as e:               # an id map needs kept paths
        with pytest.raises(agx.AgxError) as x:
            e.unitigs(edge_support=True, id_map=True)
        assert x.value.code == agx.AGX_E_ARG and "AGX_FLAG_KEEP_PATHS" in x.value.msg
    with unit(keep_counts=True, keep_paths=True, edge_support=True) as e:
        a, b = e.unitigs(edge_support=True, id_map=True), e.unitigs(id_map=True)
        for k in ("id_first", "id_last", "seg", "rank_first"):
            assert np.array_equal(a["id_map"][k], b["id_map"][k]), k
        assert len(a["link_support"]) == len(a["link_from"])


def test_memory_without_and_with_the_flag(agx, modelled):
    """Without the flag a unit plans and holds what it did before a flagged unit lived in the process, whatever its other flags; with it, the plan grows by the
    counters: four bytes per inline edge slot of every planned node slot at least."""
    u, tmp, g, front, model = modelled("seed201")

    def measure(flags):
        with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, flags=flags) as e:
            e.load_files(tmp, 0)
            need = e.hbm_needed()
            e.upload()
            e.build()
            st = e.stats()
            if flags & agx.AGX_FLAG_EDGE_SUPPORT:
                e.edge_support()
            return need, st["device_bytes"]
    before = {f: measure(f) for f in (0, agx.AGX_FLAG_KEEP_COUNTS)}
    flagged = {f: measure(f | agx.AGX_FLAG_EDGE_SUPPORT) for f in (0, agx.AGX_FLAG_KEEP_COUNTS)}
    after = {f: measure(f) for f in (0, agx.AGX_FLAG_KEEP_COUNTS)}
    assert before == after
    n_pos = int(g["n_pos"])
    planned = (n_pos + n_pos // 4 + 4096) + (n_pos // 8 + 65536)      # the first guess of the node pool (agx_engine.cpp: plan_capacities): main slices + spill area
    for f in before:
        assert flagged[f][0] - before[f][0] >= 4 * MAXE * planned, (f, flagged[f], before[f])
        assert flagged[f][1] >= before[f][1]
