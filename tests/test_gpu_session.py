"""The on-request calls of a built unit (csrc/agx_export.cpp) behind one another and over scratch they must not trust.  All eleven kinds carve their layouts over one
device buffer and clear by hand what their kernels add into; the per-kind files call one kind on a fresh unit, where a missing clear finds zeros or its own leftovers.
Here, on the units and with the models and comparators of tests/session_calls.py (integer and byte equality throughout):

  pairs     every ordered pair (a, b) of the kinds, b == a too: a, then b, and b's answer is the model's — the junk is a's true leftover
  poison    agx_test_poison over the scratch and the edge counters — bytes 0x00, 0xFF, 0xA5 and random words — then the call; the kinds that read the counters once
            more right behind a build(), when the counters are scratch too
  chunks    the forced chunks of the per-kind files (AGX_EVIDENCE_CHUNK, AGX_SPAN_BASE_CHUNK, AGX_SPAN_CHUNK, AGX_EDGE_READS_CHUNK, AGX_LINKS_SLOTS at sizes that force
            further passes) over poison: the clears per chunk and per pass
  sessions  four seeded orders of all kinds on one unit with a reprune(coverage + 2) and a finish() behind the sixth call; one with every capacity too small, one on a
            unit without kept paths, one without edge counters (what those refuse is asked all the same); then the finish's bytes and the graph are the oracle's and
            hbm_needed() and device_bytes are what they were after the first call that took the scratch
  the hook  refused on an unbuilt, a trimmed and a count-less unit with the next answer unchanged; valid counters are left alone; a poison alone changes no finish

One build per unit serves pairs, poison and chunks."""
import contextlib
import os
import random

import numpy as np
import pytest

import links_model as LM
import session_calls as SC
from conftest import graph_mismatch
from test_gpu_links import cut_table

pytestmark = pytest.mark.gpu

UNITS = SC.units()
NAMES = list(UNITS)
PAIR_UNITS = ("seed201", "edge_overflow")
SESSION_UNIT = "edge_overflow"
PATTERNS = (0, 1, 2, 3)
KEYS = ("initial", "pre", "extended")


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


@pytest.fixture(scope="module")
def modelled(built, tmp_path_factory):
    made = {}

    def get(name, coverage=None):
        if (name, coverage) not in made:
            u = UNITS[name]
            if coverage is None:
                made[(name, None)] = SC.make_model(u, u.write(str(tmp_path_factory.mktemp(name))))
            else:
                base = get(name)
                made[(name, coverage)] = SC.make_model(u, base["tmp"], coverage, base)
        return made[(name, coverage)]
    return get


def built_unit(agx, m, **kw):
    u = m["u"]
    flags = dict(keep_counts=True, keep_paths=True, edge_support=True)
    flags.update(kw)
    e = agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, **flags)
    e.load_files(m["tmp"], 0)
    e.upload()
    e.build()
    return e


@pytest.fixture(scope="module")
def unit_of(agx, modelled):
    """name -> the resident unit, built once and finished once (the walk's kept stretches are the executor's)"""
    made = {}
    with contextlib.ExitStack() as stack:
        def get(name):
            if name not in made:
                m = modelled(name)
                e = stack.enter_context(built_unit(agx, m))
                assert e.finish()["pre"] == m["o"]["pre"]
                w = e.walk_paths()
                for k in ("rec_len", "st_off", "id_first", "id_last", "base_off", "joined"):
                    assert np.array_equal(w[k], m["w"][k]), k
                made[name] = e
            return made[name]
        yield get


def poison(agx, e, what, pattern, seed=0):
    assert agx.lib().agx_test_poison(e._h, what, pattern, seed) == agx.AGX_OK, agx.lib().agx_unit_error(e._h)


def forced(env, call, *a, **kw):
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return call(*a, **kw)
    finally:
        for k in env:
            del os.environ[k]


def check(kind, got, what):
    x = kind.same(got, kind.want())
    assert x is None, "%s: %s" % (what, x)


def test_units_and_kinds(modelled):
    """Every kind runs on every unit: on two at least, one of them with overflow edges — by the executor's record of its appends, not by the device's count."""
    assert len(NAMES) >= 2 and modelled("edge_overflow")["n_ovf"] > 0 and set(PAIR_UNITS) <= set(NAMES)
    assert any(modelled(n)["n_ovf"] > 0 for n in PAIR_UNITS) and modelled(SESSION_UNIT)["n_ovf"] > 0


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", SC.KINDS)
@pytest.mark.parametrize("name", PAIR_UNITS)
def test_every_ordered_pair(unit_of, modelled, name, a):
    kinds, e = SC.table(modelled(name)), unit_of(name)
    for b in SC.KINDS:
        kinds[a].call(e)
        check(kinds[b], kinds[b].call(e), "%s: %s behind %s" % (name, b, a))


# ---- poison -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_poison_then_call(agx, unit_of, modelled, name, kind):
    k, e = SC.table(modelled(name))[kind], unit_of(name)
    for p in PATTERNS:
        poison(agx, e, 3, p, 0x5EED0000 + 16 * SC.KINDS.index(kind) + p)
        check(k, k.call(e), "%s: %s over pattern %d" % (name, kind, p))


@pytest.mark.parametrize("kind", SC.READS_SUPPORT)
@pytest.mark.parametrize("name", NAMES)
def test_poison_behind_a_build(agx, unit_of, modelled, name, kind):
    """Behind a build the counters are the build before's: scratch, and poisoned with it.  The first call that reads them counts them again."""
    k, e = SC.table(modelled(name))[kind], unit_of(name)
    for p in PATTERNS:
        e.build()
        assert e.stats()["n_support_events"] == 0
        poison(agx, e, 3, p, 0xB0000000 + 16 * SC.KINDS.index(kind) + p)
        check(k, k.call(e), "%s: %s behind a build over pattern %d" % (name, kind, p))
        assert e.stats()["n_support_events"] == modelled(name)["sup"]["n_events"]


# ---- chunks -----------------------------------------------------------------------------------------------------------------------------------------------------

CHUNKED = {"evidence": {"AGX_EVIDENCE_CHUNK": 64}, "walk_span": {"AGX_SPAN_BASE_CHUNK": 64, "AGX_SPAN_CHUNK": 100}, "pair_span": {"AGX_SPAN_CHUNK": 100},
           "edge_reads": {"AGX_EDGE_READS_CHUNK": 1}}


@pytest.mark.parametrize("kind", list(CHUNKED))
@pytest.mark.parametrize("name", NAMES)
def test_forced_chunks_over_poison(agx, unit_of, modelled, name, kind):
    k, e = SC.table(modelled(name))[kind], unit_of(name)
    for p in (0, 1, 3):
        poison(agx, e, 3, p, 0xC0000000 + p)
        check(k, forced(CHUNKED[kind], k.call, e), "%s: %s in chunks %s over pattern %d" % (name, kind, CHUNKED[kind], p))


def links_asks(m):
    """(label, table, min_pairs, slots, passes) of the forced slot counts: `interleaved` in 4 and in 2 slots — a record of it has two links at most, so the halving always
    ends — and the per-kind file's table of single-base records cut to K links in K / 2 slots, where no record alone has more.  passes: how many the model's links force
    at least (a pass that does not fit is discarded and its range halved: three for the first split)."""
    tab = m["tables"]["interleaved"]
    n = LM.mate_links(m["frags"], m["n_pos"], m["side_xpos"], tab, 1)["n_links_all"]
    out = [("interleaved in %d slots" % s, tab, 1, s, 3 if n > s else 1) for s in (4, 2)]
    cut, k = cut_table(m)
    if cut is not None:
        a = LM.mate_links(m["frags"], m["n_pos"], m["side_xpos"], cut, 1)["a"]
        if int(np.bincount(a, minlength=1).max()) <= k // 2:
            out.append(("%d single-base links in %d slots" % (k, k // 2), cut, 2, k // 2, 3))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_forced_link_slots_over_poison(agx, unit_of, modelled, name):
    """Where `if (first)` and the per-pass clears are decided: the later passes find the first pass's table, flags and compacted rows."""
    m, e = modelled(name), unit_of(name)
    for label, tab, t, slots, passes in links_asks(m):
        want = LM.mate_links(m["frags"], m["n_pos"], m["side_xpos"], tab, t)
        for p in (0, 1, 3):
            poison(agx, e, 3, p, 0x11000000 + p)
            got = forced({"AGX_LINKS_SLOTS": slots}, e.mate_links, tab, t)
            x = SC._links(got, want)
            assert x is None, "%s: %s over pattern %d: %s" % (name, label, p, x)
            assert got["n_slots"] == slots and got["n_passes"] >= passes, (name, label, got["n_passes"])


def test_forced_link_slots_reach_a_second_pass(modelled):
    asks = [a for n in NAMES for a in links_asks(modelled(n))]
    assert sum(1 for a in asks if a[4] > 1 and "interleaved" in a[0]) >= 2 and any("single-base" in a[0] for a in asks), [a[0] for a in asks]


# ---- sessions ---------------------------------------------------------------------------------------------------------------------------------------------------

SESSIONS = [("plain", 1, {}, {}), ("small_caps", 2, {}, {"AGX_TEST_SMALL_CAPS": "1"}), ("no_paths", 3, {"keep_paths": False}, {}), ("no_edge_support", 4, {"edge_support": False}, {})]


@pytest.mark.parametrize("label,seed,flags,env", SESSIONS, ids=[s[0] for s in SESSIONS])
def test_whole_session(agx, modelled, monkeypatch, label, seed, flags, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    order = list(SC.KINDS)
    random.Random(seed).shuffle(order)
    m = modelled(SESSION_UNIT)
    support = flags.get("edge_support", True)
    refused = (SC.NEEDS_PATHS if not flags.get("keep_paths", True) else ()) + (SC.NEEDS_SUPPORT if not support else ())
    held = None
    with built_unit(agx, m, **flags) as e:
        if env:
            assert e.stats()["build_attempts"] > 1, "the pool did not grow under AGX_TEST_SMALL_CAPS"
        assert e.finish()["pre"] == m["o"]["pre"]
        for i, kind in enumerate(order):
            if i == 6:
                e.reprune(m["cov"] + 2)
                m = modelled(SESSION_UNIT, m["cov"] + 2)
                assert e.finish()["pre"] == m["o"]["pre"]
            k = SC.table(m, support)[kind]
            what = "%s: call %d, %s behind %s" % (label, i, kind, order[i - 1] if i else "the build")
            if kind in refused:
                with pytest.raises(agx.AgxError) as x:
                    k.call(e)
                assert x.value.code == agx.AGX_E_ARG, what
                continue
            check(k, k.call(e), what)
            if held is None and kind != "edge_support":      # (edge support alone takes none of the export's scratch)
                held = (e.hbm_needed(), e.stats()["device_bytes"])
        assert graph_mismatch(m["g"], e.graph()) is None
        out = e.finish()
        for key in KEYS:
            assert out[key] == m["o"][key], (label, key)
        assert (e.hbm_needed(), e.stats()["device_bytes"]) == held, label
    assert len(set(refused)) == {"plain": 0, "small_caps": 0, "no_paths": 1, "no_edge_support": 3}[label]


# ---- the hook ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_hook_is_refused_where_an_export_is(agx, modelled):
    m = modelled("walk_kinds")
    u = m["u"]
    L = agx.lib()
    whole = SC.table(m)["unitigs"]
    with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage, keep_counts=True) as e:
        e.load_files(m["tmp"], 0)
        e.upload()
        assert L.agx_test_poison(e._h, 3, 1, 0) == agx.AGX_E_ARG and b"not built" in L.agx_unit_error(e._h)      # unbuilt
        e.build()
        for what, pattern in ((4, 0), (1, 4)):
            assert L.agx_test_poison(e._h, what, pattern, 0) == agx.AGX_E_ARG
        check(whole, whole.call(e), "behind the refusals")
        e.download()
        e.trim()
        assert L.agx_test_poison(e._h, 3, 1, 0) == agx.AGX_E_ARG and b"not built" in L.agx_unit_error(e._h)      # trimmed
        out = e.finish()
        for key in KEYS:
            assert out[key] == m["o"][key], key
    with agx.Unit(k=u.k, insert_variation=u.iv, coverage=u.coverage) as e:                                          # keeps no counts
        e.load_files(m["tmp"], 0)
        e.upload()
        e.build()
        before = e.stats()["device_bytes"]
        assert L.agx_test_poison(e._h, 3, 1, 0) == agx.AGX_E_ARG and b"KEEP_COUNTS" in L.agx_unit_error(e._h)
        assert e.stats()["device_bytes"] == before
        out = e.finish()
        for key in KEYS:
            assert out[key] == m["o"][key], key
    assert L.agx_test_poison(None, 3, 1, 0) == agx.AGX_E_ARG


@pytest.mark.parametrize("name", ["seed203", "edge_overflow"])
def test_hook_leaves_valid_counters_and_the_finish(agx, modelled, name):
    m = modelled(name)
    with built_unit(agx, m) as e:
        for p in PATTERNS:      # a poison alone, of everything: nothing a build or a walk reads
            poison(agx, e, 3, p, 77)
        out = e.finish()
        for key in KEYS:
            assert out[key] == m["o"][key], key
        need, held = e.hbm_needed(), e.stats()["device_bytes"]
        e.unitigs()
        assert (e.hbm_needed(), e.stats()["device_bytes"]) == (need, held), "the hook took the buffer as an export takes it"
        first, events = e.edge_support(), e.stats()["n_support_events"]
        assert events == m["sup"]["n_events"] > 0
        for p in PATTERNS:
            poison(agx, e, 2, p, 78)
            again = e.edge_support()
            for k in ("edge_start", "edge_dst", "edge_cnt"):
                assert np.array_equal(first[k], again[k]), (k, p)
            assert e.stats()["n_support_events"] == events and (again["n_events"], again["n_contributions"]) == (first["n_events"], first["n_contributions"])
        check(SC.table(m)["support"], SC.table(m)["support"].call(e), "the link support behind a poison of valid counters")
        assert e.finish() == out
