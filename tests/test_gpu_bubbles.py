"""The bubbles on the MI355X (-m gpu): Unit.bubbles() (agx_unit_bubbles, agx_bubbles.hip) against tests/bubbles_model.py applied to the region
model's table of the oracle's graph, and against the host-only twin applied to what Unit.unitigs() gives for the same window — on the units and windows
tests/test_bubbles_cases.py runs on the CPU, one build per unit (kept counts, edge support).  With and without support (the numbers against
tests/edge_support_model.py), max_nodes, a second call, calls after reprune and after finish, every refusal with the unit unchanged behind it, hbm_needed() and
device_bytes, a plain export before and after, and the finish's bytes behind it all.  Every comparison is integer equality."""
import contextlib
import os

import numpy as np
import pytest

import bubbles_model as BM
import bubbles_units as BU
import edge_support_model as ESM
import harness as H
import lean_units as LU
import unitig_region_model as R
import unitig_units as UU
import walk_units as WU
from hostsim import sim
from test_bubbles_cases import SEEDS
from test_gpu_parity import CONFIGS

pytestmark = pytest.mark.gpu
UNITIG_CASES = {c.name: c for c in UU.cases()}
UNITS = {u.name: u for u in BU.units()}
KEYS = ("initial", "pre", "extended")
TABLE = BM.PER_BUBBLE + BM.PER_BRANCH


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


class Made:
    """One unit: its files, the oracle's run, the expected tables (made once, never changed) and the built unit."""

    def __init__(self, agx, tmp, k, iv, coverage, stack):
        self.tmp, self.k, self.iv, self.coverage = tmp, k, iv, coverage
        self.o = H.run_oracle(tmp, 0, k, iv, coverage, graph=True)
        self.g = self.o["graph"]
        self.n, self.ref = int(self.g["n_pos"]), bytes(self.g["pos_nuc"])
        self._t, self._sup = {}, None
        self.u = stack.enter_context(agx.Unit(k=k, insert_variation=iv, coverage=coverage, keep_counts=True, edge_support=True))
        self.u.load_files(tmp, 0)
        self.u.upload()
        self.u.build()

    def window(self, w):
        return (w[0], min(w[1], self.n), w[2])

    def table(self, w):
        if w not in self._t:
            self._t[w] = R.region_unitigs(self.g, w[0], w[1], w[2], self.ref)
        return self._t[w]

    def link_support(self, w):
        """the support of every link of the window's table, from tests/edge_support_model.py on the executor's front: tail node -> head node, as the piece model has them"""
        if self._sup is None:
            self._sup = ESM.support(sim.run(self.tmp, 0, self.k, self.iv, self.coverage, front=True)["front"], self.g, self.k, self.iv)
        P, t = UU.piece_model(self.g, *w), self.table(w)
        head = [int(P.node[h]) for h in P.heads]
        tail = [int(P.node[int(P.starts[ch[-1]] + P.p_len[ch[-1]] - 1)]) for ch in P.chains]
        want = [ESM.edge_support_of(self._sup, tail[a], head[b]) for a, b in zip(np.asarray(t["link_from"]).tolist(), np.asarray(t["link_to"]).tolist())]
        assert None not in want, w
        return want


@pytest.fixture(scope="module")
def made(agx, built, tmp_path_factory):
    out = {}
    with contextlib.ExitStack() as stack:
        def get(kind, name):
            if (kind, name) not in out:
                if kind == "seed":
                    cfg = next(c for c in CONFIGS if c["seed"] == name)
                    run = H.synth(str(tmp_path_factory.mktemp("run%d" % name) / "run"), sam_seq=0, **cfg)
                    meta = H.read_meta(run)
                    out[(kind, name)] = Made(agx, os.path.join(run, "tmp"), meta["k"], meta["insert_variation"], meta["coverage"], stack)
                else:
                    c = UNITIG_CASES[name] if kind == "unitig" else UNITS[name]
                    out[(kind, name)] = Made(agx, WU.write_unit(c.unit, str(tmp_path_factory.mktemp(name))), LU.K, c.iv, c.coverage, stack)
            return out[(kind, name)]
        yield get


def ask(m, w, **kw):
    return m.u.bubbles(region=(w[0], w[1]), min_coverage=w[2], **kw)


def same(got, want, what):
    x = BM.mismatch(got, want)
    assert x is None, "%s: %s" % (what, x)


def same_arrays(a, b, what):
    """two answers of the library's are one"""
    for f in BM.TOTALS + TABLE + (BM.SUPPORT if a["has_support"] else ()):
        assert np.array_equal(a[f], b[f]), "%s: %s" % (what, f)
    assert a["has_support"] == b["has_support"] and bytes(a["seq"]) == bytes(b["seq"]), what


@pytest.mark.parametrize("name", list(UNITIG_CASES))
def test_unitig_cases(agx, made, name):
    m, case = made("unitig", name), UNITIG_CASES[name]
    for i, w in enumerate(case.windows):
        what = "%s: window [%d, %d) at %d" % (name, w[0], w[1], w[2])
        got = ask(m, w)
        same(got, BM.bubbles(m.table(w)), what)
        if i % 4 == 0:
            t = m.u.unitigs(region=(w[0], w[1]), min_coverage=w[2], edge_support=True)
            same_arrays(ask(m, w, edge_support=True), agx.unitigs_bubbles(t, t["link_support"]), what + ", the twin on the export")
            same_arrays(ask(m, w, max_nodes=1), agx.unitigs_bubbles(t, None, 1), what + ", max_nodes 1")


@pytest.mark.parametrize("name", list(UNITS))
def test_hand_made_units(agx, made, name):
    m, u = made("unit", name), UNITS[name]
    seen = {}
    for w0 in u.windows:
        w = m.window(w0)
        what = "%s: window [%d, %d) at %d" % (name, w[0], w[1], w[2])
        t = m.table(w)
        want = BM.bubbles(t)
        got = ask(m, w)
        same(got, want, what)
        assert got["ms"] > 0.0 and agx.bubbles_tsv(got, 2) == BM.tsv(want, 2), what
        same(ask(m, w, max_nodes=0), BM.bubbles(t, None, 0), what + ", max_nodes 0")
        if u.support:
            sup = m.link_support(w)
            same(ask(m, w, edge_support=True), BM.bubbles(t, sup), what + ", with support")
            same(ask(m, w), want, what + ", without support behind a call with it")
        seen[w0] = (want, t)
    for desc, w0, fn in u.want:
        assert fn(*seen[w0]), "%s: window %s: %s" % (name, w0, desc)


@pytest.mark.parametrize("seed", list(SEEDS))
def test_generated_units(agx, made, seed):
    m = made("seed", seed)
    before = m.u.unitigs(region=(0, m.n), min_coverage=0)
    for cov in (0, 5):
        w = (0, m.n, cov)
        t = m.table(w)
        got = ask(m, w)
        same(got, BM.bubbles(t), "seed%d at %d" % (seed, cov))
        same_arrays(ask(m, w), got, "seed%d at %d, a second call" % (seed, cov))
        tu = m.u.unitigs(region=(0, m.n), min_coverage=cov, edge_support=True)
        same_arrays(ask(m, w, edge_support=True), agx.unitigs_bubbles(tu, tu["link_support"]), "seed%d at %d, the twin on the export" % (seed, cov))
        for mx in (1, int(got["longest_branch"]) - 1, int(got["longest_branch"])):
            same(ask(m, w, max_nodes=mx), BM.bubbles(t, None, mx), "seed%d at %d, max_nodes %d" % (seed, cov, mx))
        if cov == 0:
            assert tuple(int(got[f]) for f in ("n_segs", "n_links", "n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared")) == SEEDS[seed][0]
            assert got["bytes_down"] > 0
        else:
            assert int(got["n_bubbles_all"]) == SEEDS[seed][1]
    if seed == 203:
        assert len(before["head_pos"]) > 4096, "the scans take a second level"
    after = m.u.unitigs(region=(0, m.n), min_coverage=0)
    assert UU.table_mismatch(after, before) is None and UU.table_mismatch(after, m.table((0, m.n, 0))) is None, "a plain export before and after"


def test_reprune_finish_and_what_stays(agx, made):
    """Behind a reprune the explicit thresholds answer as before and the unit's own threshold is the new one; behind a finish the call still runs; hbm_needed() and
    device_bytes are what they were after the first export; agx_stats has no field of the call's; the finish's bytes are the oracle's."""
    m = made("unit", "chain")
    w = (0, m.n, 1)
    m.u.unitigs()
    need, held, fields = m.u.hbm_needed(), m.u.stats()["device_bytes"], list(m.u.stats())
    first = ask(m, w)
    same(m.u.bubbles(), BM.bubbles(m.table(w)), "no window, the unit's own coverage")
    try:
        m.u.reprune(20)
        same_arrays(ask(m, w), first, "an explicit threshold behind a reprune")
        same(m.u.bubbles(), BM.bubbles(m.table((0, m.n, 20))), "the unit's own coverage behind a reprune")
    finally:
        m.u.reprune(m.coverage)
    out = m.u.finish()
    for key in KEYS:
        assert out[key] == m.o[key], key
    same_arrays(ask(m, w), first, "behind a finish")
    assert m.u.hbm_needed() == need and m.u.stats()["device_bytes"] == held and list(m.u.stats()) == fields and fields[-1] == "ms_walk_span"
    assert m.u.finish() == out


def test_refusals_leave_the_unit_as_it_was(agx, made):
    m = made("unit", "kinds")
    w = (BU.XS - 100, BU.XS + 100, 1)
    want = BM.bubbles(m.table(w))

    def unit(build=True, **kw):
        flags = dict(keep_counts=True, edge_support=True)
        flags.update(kw)
        e = agx.Unit(k=LU.K, insert_variation=m.iv, coverage=m.coverage, **flags)
        e.load_files(m.tmp, 0)
        e.upload()
        if build:
            e.build()
        return e

    def refused(e, what, *a, **kw):
        with pytest.raises(agx.AgxError) as x:
            e.bubbles(*a, **kw)
        assert x.value.code == agx.AGX_E_ARG and what in x.value.msg, x.value.msg

    with unit() as e:
        fin = e.finish()
        same(e.bubbles(region=w[:2], min_coverage=1, edge_support=True), BM.bubbles(m.table(w), m.link_support(w)), "a unit of its own")
        held = e.stats()["device_bytes"]
        refused(e, "is not within the unit's positions", region=(5, 4), min_coverage=1)
        refused(e, "is not within the unit's positions", region=(0, m.n + 1), min_coverage=1)
        with pytest.raises(agx.AgxError):
            e.bubbles(max_nodes=1 << 32)
        with pytest.raises(agx.AgxError):
            e.bubbles(min_coverage=-1)
        assert e.stats()["device_bytes"] == held and e.finish() == fin
        same(e.bubbles(region=w[:2], min_coverage=1), want, "behind the refusals")
        e.download()
        refused(e, "not built", edge_support=True)                       # (the counting reads arrays a download gives away)
        same(e.bubbles(region=w[:2], min_coverage=1), want, "downloaded, without support")
        e.trim()
        refused(e, "not built")
        assert e.finish() == fin
    with unit() as e:
        e.release()
        refused(e, "not built")
    with unit(build=False) as e:
        refused(e, "not built")
        e.build()
        same(e.bubbles(region=w[:2], min_coverage=1), want, "built behind a refusal")
        assert e.finish() == fin
    with unit(keep_counts=False, edge_support=False) as e:
        held = e.stats()["device_bytes"]
        refused(e, "AGX_FLAG_KEEP_COUNTS")
        assert e.stats()["device_bytes"] == held and e.finish() == fin
    with unit(edge_support=False) as e:
        held = e.stats()["device_bytes"]
        refused(e, "AGX_FLAG_EDGE_SUPPORT", edge_support=True)
        same(e.bubbles(region=w[:2], min_coverage=1), want, "a unit without edge support")
        assert e.finish() == fin
    with unit(flags=agx.AGX_FLAG_ONE_SHOT, edge_support=False) as e:
        same(e.bubbles(region=w[:2], min_coverage=1), want, "a one-shot unit before its finish")
        assert e.finish() == fin
        refused(e, "one-shot")
