"""Edge reads on the device (agx_k_edge_reads, agx_unit_edge_reads) against tests/edge_reads_model.py on the units of
tests/test_gpu_edge_support.py: every case of tests/edge_units.py and the generated seeds 201 and 203.  Per unit one build serves every check — the whole unit, the
thresholds, the windows, forced chunks, a second call, a second build of the resident unit, a reprune and the finish behind it —, each answer compared whole, field by
field, with the model's table.  The overflow cases also run with every capacity starting small, the window cases with the upload cut in three, and two units in the
file-order upload form, where perm[] is uploaded and not written by agx_k_hit_prep."""
import os

import numpy as np
import pytest

import edge_reads_model as ERM
from test_edge_support_cases import EDGE_UNITS, SEED_UNITS, UNITS, modelled  # noqa: F401  (modelled: the module fixture)
from test_edge_reads_cases import windows

pytestmark = pytest.mark.gpu

NAMES = [u.name for u in EDGE_UNITS + SEED_UNITS] + ["lean_general"]      # (lean_general: the unit whose tile lists hold GENERAL lean records)
ALL = ERM.ALL
FIELDS = ERM.EDGE_KEYS + ("hit_off", "hit")


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


@pytest.fixture(scope="module")
def reads_of(modelled):
    made = {}

    def get(name):
        if name not in made:
            u, tmp, g, front, model = modelled(name)
            made[name] = ERM.reads(front, g, u.k, u.iv)
        return made[name]
    return get


def same(got, want):
    for k in FIELDS:
        assert np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), k
        assert got[k].dtype == (np.uint64 if k == "hit_off" else np.uint32), k


def named_edge(rd, g):
    """The edge every unit is asked for by its support: the first, in canonical order, of the largest support"""
    s = max(len(h) for h in rd.values())
    e = min(e for e, h in rd.items() if len(h) == s)
    (sp, dp), (sv, dv) = ERM.pos_var(g, list(e))
    return (int(sp), int(sv), int(dp), int(dv)), s


def jump_edge(rd, g):
    """An edge that skips positions (None: the unit has none): the first in canonical order"""
    for e in sorted(rd):
        (sp, dp), (sv, dv) = ERM.pos_var(g, list(e))
        if dp > sp + 1:
            return int(sp), int(sv), int(dp), int(dv)
    return None


def has_edge(t, e):
    return e in set(zip(t["src_pos"].tolist(), t["src_var"].tolist(), t["dst_pos"].tolist(), t["dst_var"].tolist()))


def asked(rd, g):
    """(label, lo, hi, max_support) of everything a unit is asked for after its first build"""
    n_pos = int(g["n_pos"])
    e, s = named_edge(rd, g)
    out = [("whole", 0, n_pos, ALL), ("none", 0, n_pos, 0), ("one", 0, n_pos, 1), ("below", 0, n_pos, s - 1), ("at", 0, n_pos, s)]
    out += [("w%d_%d" % (i, top), lo, hi, top) for i, (lo, hi) in enumerate(windows(n_pos)) for top in (ALL, 1)]
    j = jump_edge(rd, g)
    if j is not None:      # a window whose only position is the jump's source; one that ends on the source, one that starts on the target
        out += [("jump_src", j[0], j[0] + 1, ALL), ("jump_ends_on_src", max(j[0] - 70, 0), j[0] + 1, ALL), ("jump_starts_on_dst", j[2], min(j[2] + 70, n_pos), ALL)]
    return out


def with_env(key, value, fn):
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


def run_engine(agx, u, tmp, rd, g, full=True):
    """One build of the unit with both flags; everything the tests look at, collected before the unit goes."""
    out = {"asked": {}}
    with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, keep_counts=True, edge_support=True) as e:
        e.load_files(tmp, 0)
        e.upload()
        e.build()
        e.gfa(0)      # an export first: the unit then holds the export's buffer (a unit whose pool grew in the build takes the difference there), which the calls below share
        out["need0"] = e.hbm_needed()
        out["stats0"] = e.stats()
        out["whole"] = e.edge_reads()
        out["stats1"] = e.stats()
        out["need1"] = e.hbm_needed()
        out["graph"], out["support"] = e.graph(), e.edge_support()
        for label, lo, hi, top in asked(rd, g):
            out["asked"][label] = (lo, hi, top, e.edge_reads((lo, hi), top))
        if full:
            out["second"] = e.edge_reads()
            out["chunk1"] = with_env("AGX_EDGE_READS_CHUNK", "1", e.edge_reads)
            out["chunk2"] = with_env("AGX_EDGE_READS_CHUNK", "2", e.edge_reads)
            n_pos = int(g["n_pos"])
            mid = (n_pos // 3 + 5, 2 * n_pos // 3 + 9)
            out["chunk1_mid"] = (mid, with_env("AGX_EDGE_READS_CHUNK", "1", lambda: e.edge_reads(mid, 2)), e.edge_reads(mid, 2))
            out["stats2"] = e.stats()
            e.build()
            out["rebuilt_stats"] = e.stats()
            out["rebuilt"] = e.edge_reads()
            e.reprune(u.coverage + 2)
            out["repruned"] = e.edge_reads()
            out["repruned_one"] = e.edge_reads(None, 1)
            out["stats3"] = e.stats()
            out["finish"] = e.finish()
    return out


@pytest.fixture(scope="module")
def engine_of(agx, modelled, reads_of):
    made = {}

    def get(name):
        if name not in made:
            u, tmp, g, front, model = modelled(name)
            made[name] = run_engine(agx, u, tmp, reads_of(name), g)
        return made[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_whole_unit(engine_of, modelled, reads_of, name):
    u, tmp, g, front, model = modelled(name)
    e, rd = engine_of(name), reads_of(name)
    t = e["whole"]
    same(t, ERM.table(rd, g))
    assert len(t["hit"]) == int(t["hit_off"][-1]) == e["support"]["n_contributions"] == model["n_contributions"]
    assert np.array_equal(np.diff(t["hit_off"].astype(np.int64)), t["support"].astype(np.int64)), "an edge that does not list exactly `support` hits"
    # the edge set is agx_unit_graph's, in its order, and the numbers are agx_unit_edge_support's
    gr, ns = e["graph"], e["graph"]["node_start"].astype(np.int64)
    src = np.repeat(np.arange(int(gr["n_nodes"])), np.diff(gr["edge_start"].astype(np.int64)))
    assert np.array_equal(ns[t["src_pos"].astype(np.int64)] + t["src_var"], src) and np.array_equal(ns[t["dst_pos"].astype(np.int64)] + t["dst_var"], gr["edge_dst"])
    assert np.array_equal(t["support"], e["support"]["edge_cnt"])
    assert int(t["hit"].max()) < len(front["dhit"])


@pytest.mark.parametrize("name", NAMES)
def test_thresholds_and_windows(engine_of, modelled, reads_of, name):
    u, tmp, g, front, model = modelled(name)
    e, rd = engine_of(name), reads_of(name)
    for label, (lo, hi, top, t) in e["asked"].items():
        try:
            same(t, ERM.table(rd, g, lo, hi, top))
        except AssertionError as x:
            raise AssertionError("%s [%d, %d) <= %d: %s" % (label, lo, hi, top, x))
        assert ((t["src_pos"] >= lo) & (t["src_pos"] < hi)).all() and (t["support"] <= top).all()
    a = e["asked"]
    assert len(a["none"][3]["src_pos"]) == 0 and len(a["w1_1"][3]["src_pos"]) == 0 and len(a["w1_%d" % ALL][3]["hit"]) == 0      # threshold 0, the empty window
    edge, s = named_edge(rd, g)
    assert has_edge(a["at"][3], edge) and not has_edge(a["below"][3], edge)
    assert (a["one"][3]["support"] == 1).all()


@pytest.mark.parametrize("name", [n for n in NAMES if n in ("edge_jump", "edge_jump_windows", "edge_overflow", "edge_sweep_slow")])
def test_an_event_belongs_to_its_source(engine_of, modelled, reads_of, name):
    u, tmp, g, front, model = modelled(name)
    e, rd = engine_of(name), reads_of(name)
    j = jump_edge(rd, g)
    assert j is not None
    a = e["asked"]
    t = a["jump_src"][3]
    assert has_edge(t, j) and (t["dst_pos"] >= a["jump_src"][1]).all(), "the window's only events jump out of it"
    assert has_edge(a["jump_ends_on_src"][3], j) and not has_edge(a["jump_starts_on_dst"][3], j)


def test_both_paths_and_general_records(engine_of, modelled, reads_of):
    """edge_register: single -> single lanes and positions with several variants; edge_general: whole positions resolved hit by hit (two conti-mers, five variants);
    lean_general: tile lists with GENERAL lean records, which edge_general's lists do not hold.  The whole answers are the model's (test_whole_unit)."""
    for name in ("edge_register", "edge_general"):
        u, tmp, g, front, model = modelled(name)
        t = engine_of(name)["whole"]
        per_pos = np.diff(g["node_start"].astype(np.int64))
        assert (t["src_var"] > 0).any() and (t["dst_var"] > 0).any() and (per_pos[t["src_pos"].astype(np.int64)] == 1).any()
    kinds = modelled("lean_general")[3]["tile_recs"]["geo"].astype(np.int64) >> 30
    assert (kinds == 0).any(), "lean_general lost its GENERAL records"
    assert len(engine_of("lean_general")["whole"]["hit"]) == modelled("lean_general")[4]["n_contributions"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_chunks_second_call_rebuild_and_reprune(engine_of, modelled, reads_of, name):
    u, tmp, g, front, model = modelled(name)
    e, rd = engine_of(name), reads_of(name)
    for k in ("second", "chunk1", "chunk2", "rebuilt", "repruned"):
        try:
            same(e[k], e["whole"])
        except AssertionError as x:
            raise AssertionError("%s: %s" % (k, x))
    mid, forced, plain = e["chunk1_mid"]
    same(forced, plain)
    same(plain, ERM.table(rd, g, mid[0], mid[1], 2))
    same(e["repruned_one"], e["asked"]["one"][3])
    assert e["rebuilt_stats"]["n_support_events"] == 0, "a build leaves the counters of the build before it"


@pytest.mark.parametrize("name", NAMES)
def test_stats_memory_and_finish(agx, engine_of, modelled, name):
    u, tmp, g, front, model = modelled(name)
    e = engine_of(name)
    assert e["stats0"]["ms_edge_reads"] == 0.0 and e["stats1"]["ms_edge_reads"] > 0.0
    assert e["stats0"]["n_support_events"] == 0 and e["stats1"]["n_support_events"] == model["n_events"]      # the counters were made by the first call
    assert e["need0"] == e["need1"]
    assert e["stats0"]["device_bytes"] == e["stats1"]["device_bytes"] == e["stats2"]["device_bytes"]      # the calls take nothing beyond what an export takes
    assert e["rebuilt_stats"]["device_bytes"] == e["stats3"]["device_bytes"]                                # nor after the second build and the reprune
    with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage + 2, keep_counts=True, edge_support=True) as p:      # never asked: what its finish gives
        p.load_files(tmp, 0)
        p.upload()
        p.build()
        p.gfa(0)
        assert p.hbm_needed() == e["need0"] and p.stats()["device_bytes"] == e["stats0"]["device_bytes"]
        assert p.finish() == e["finish"]


@pytest.mark.parametrize("name", [n for n in NAMES if UNITS[n].overflow])
def test_overflow_case_small_caps(agx, modelled, reads_of, name, monkeypatch):
    u, tmp, g, front, model = modelled(name)
    monkeypatch.setenv("AGX_TEST_SMALL_CAPS", "1")
    e = run_engine(agx, u, tmp, reads_of(name), g, full=False)
    assert e["stats1"]["build_attempts"] > 1 and e["stats1"]["n_edge_overflow"] > 4
    same(e["whole"], ERM.table(reads_of(name), g))
    for label, (lo, hi, top, t) in e["asked"].items():
        same(t, ERM.table(reads_of(name), g, lo, hi, top))


def test_overflow_dup_filter_reads_the_first_entry(engine_of, modelled, reads_of):
    u, tmp, g, front, model = modelled("edge_overflow_dup")
    e, rd = engine_of("edge_overflow_dup"), reads_of("edge_overflow_dup")
    assert e["stats1"]["n_edge_overflow"] >= 5
    x = int(np.argmax(np.bincount(e["whole"]["src_pos"].astype(np.int64))))      # the source position with the most edges: the one that overflows
    one = e["asked"]["one"][3]
    want = ERM.table(rd, g, 0, int(g["n_pos"]), 1)
    assert (want["src_pos"] == x).sum() > 4, "the overflowing source has no edges of support 1 beyond its inline slots"
    same(one, want)


@pytest.mark.parametrize("name", [n for n in NAMES if UNITS[n].windows])
def test_window_case_upload_in_three_windows(agx, modelled, reads_of, name, monkeypatch):
    u, tmp, g, front, model = modelled(name)
    monkeypatch.setenv("AGX_UPLOAD_WINDOWS", "3")
    e = run_engine(agx, u, tmp, reads_of(name), g, full=False)
    same(e["whole"], ERM.table(reads_of(name), g))
    for label, (lo, hi, top, t) in e["asked"].items():
        same(t, ERM.table(reads_of(name), g, lo, hi, top))


@pytest.mark.parametrize("name", ["edge_jump", "seed201"])
def test_file_order_upload_form(agx, modelled, reads_of, name, monkeypatch):
    u, tmp, g, front, model = modelled(name)
    monkeypatch.setenv("AGX_ROW_DIFF", "1")
    monkeypatch.setenv("AGX_NO_TILED_UPLOAD", "1")      # (rows that gain nothing as differences would cross tile-ordered: the file-order form is asked for by name as well)
    with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, keep_counts=True, edge_support=True) as e:
        e.load_files(tmp, 0)
        e.upload()
        e.build()
        f = e.front()
        t, one = e.edge_reads(), e.edge_reads(None, 1)
    assert f["tiled"] == 0 and not np.array_equal(f["perm"], np.arange(len(f["perm"])))
    same(t, ERM.table(reads_of(name), g))
    same(one, ERM.table(reads_of(name), g, 0, int(g["n_pos"]), 1))


def test_refusals(agx, modelled):
    u, tmp, g, front, model = modelled("edge_jump")
    n_pos = int(g["n_pos"])

    def unit(build=True, **kw):
        e = agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, **kw)
        e.load_files(tmp, 0)
        e.upload()
        if build:
            e.build()
        return e

    def refused(e, what, region=None):
        before = e.stats()
        with pytest.raises(agx.AgxError) as x:
            e.edge_reads(region)
        assert x.value.code == agx.AGX_E_ARG and what in x.value.msg, x.value.msg
        after = e.stats()
        assert before["device_bytes"] == after["device_bytes"] and after["ms_edge_reads"] == before["ms_edge_reads"] and after["n_support_events"] == before["n_support_events"]
    with unit(keep_counts=True) as e:
        refused(e, "AGX_FLAG_EDGE_SUPPORT")
        assert e.gfa(0)                                                # the unit is as it was
    with unit(edge_support=True) as e:
        refused(e, "AGX_FLAG_KEEP_COUNTS")
        assert e.edge_support()["n_edges"] == int(g["n_edges"])
    with unit(build=False, keep_counts=True, edge_support=True) as e:
        refused(e, "not built")
    with unit(keep_counts=True, edge_support=True, flags=agx.AGX_FLAG_ONE_SHOT) as e:
        refused(e, "one-shot")
    with unit(keep_counts=True, edge_support=True) as e:
        for region in ((5, 4), (0, n_pos + 1), (n_pos + 1, n_pos + 1)):
            refused(e, "window", region)
        want = e.edge_reads()
        assert len(e.edge_reads((n_pos, n_pos))["src_pos"]) == 0
        e.download()
        refused(e, "not built")
        e.trim()
        refused(e, "not built")
        e.upload()
        e.build()
        same(e.edge_reads(), want)                                     # again after a new upload and build
        e.release()
        refused(e, "not built")
