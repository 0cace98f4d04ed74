"""One table of the calls that answer a question about a built unit on request (csrc/agx_export.cpp): the whole unitig export, the region export, the mapped export,
the export with link support, edge support, edge reads, walk evidence, pair span, walk span, mate links and bubbles.  For a modelled unit, table(m) gives per kind
call(e) — the engine's answers, one per argument set —, want() — the plain models' answers to the same questions, made once — and same(got, want): None, or a text
that names the argument set, the field and the index.  The models and the comparators are the ones of the per-kind tests (tests/test_gpu_*.py); nothing is compared here
that they do not compare, and nothing less.  The window kinds ask for the whole unit and for a middle window; the kinds under a stretch table for the stretches of the
unit's own finish and for tests/links_units.py's "interleaved"; the evidence and the walk span at thresholds that produce intervals.

tests/test_gpu_session.py runs the kinds behind one another and over poisoned scratch; tests/test_session_calls.py checks the table itself on the CPU."""
import os

import numpy as np

import bubbles_model as BM
import bubbles_units as BU
import edge_reads_model as ERM
import edge_support_model as ESM
import evidence_model as EM
import harness as H
import lean_units as LU
import links_model as LM
import links_units as LKU
import path_model as PM
import span_model as SM
import unitig_model as M
import unitig_region_model as R
import unitig_units as UU
import walk_model as WM
import walk_units as WU
from gpu_checks import check_counts
from hostsim import sim
from test_edge_support_cases import EDGE_UNITS
from test_evidence_cases import SEED_UNITS, WALK_UNITS, executor_paths
from test_evidence_cases import thresholds as evidence_thresholds
from test_gpu_edge_reads import same as edge_reads_same
from test_gpu_edge_support import tails_of
from test_gpu_paths import same_map
from test_span_cases import thresholds as span_thresholds

KINDS = ("unitigs", "region", "mapped", "support", "edge_support", "edge_reads", "evidence", "pair_span", "walk_span", "mate_links", "bubbles")
NEEDS_PATHS = ("mapped",)                                    # refused on a unit without AGX_FLAG_KEEP_PATHS
NEEDS_SUPPORT = ("support", "edge_support", "edge_reads")    # refused on a unit without AGX_FLAG_EDGE_SUPPORT
WINDOW_KINDS = ("region", "mapped", "support", "edge_reads", "pair_span", "bubbles")
TABLE_KINDS = ("evidence", "walk_span", "mate_links")
READS_SUPPORT = ("support", "edge_support", "edge_reads", "evidence", "bubbles")      # the kinds that read the edge counters


class SessionUnit:
    def __init__(self, name, k, iv, coverage, write):
        """write(dir) -> tmp/ directory of the unit's files"""
        self.name, self.k, self.iv, self.coverage, self.write = name, k, iv, coverage, write


def _named(units, name):
    u = next(u for u in units if u.name == name)
    return SessionUnit(u.name, u.k, u.iv, u.coverage, u.write)


def units():
    """name -> unit: the generated seeds 201 and 203, the walk unit `kinds`, the edge unit `overflow` and the bubbles unit `kinds`"""
    b = next(u for u in BU.units() if u.name == "kinds")
    out = [_named(SEED_UNITS, "seed201"), _named(SEED_UNITS, "seed203"), _named(WALK_UNITS, "walk_kinds"), _named(EDGE_UNITS, "edge_overflow"),
           SessionUnit("bubbles_kinds", LU.K, b.iv, b.coverage, lambda d: WU.write_unit(b.unit, d))]
    return {u.name: u for u in out}


def make_model(u, tmp, coverage=None, base=None):
    """What the models need of a unit, made once: the oracle's run and graph, the executor's front (file order), its overflow appends and the stretches of its finish, the
    walk model's ids, the fragments and the edge-support model.  coverage, base: the same files at another coverage (the unit after agx_unit_reprune) — what does not
    depend on the threshold is base's."""
    cov = u.coverage if coverage is None else coverage
    o = H.run_oracle(tmp, 0, u.k, u.iv, cov, graph=True)
    g = o["graph"]
    if base is None:
        s = sim.run(tmp, 0, u.k, u.iv, cov, front=True, edges=True)
        front = s["front"]
        m = {"front": front, "frags": SM.fragments(front), "sup": ESM.support(front, g, u.k, u.iv), "n_ovf": len(s["ovf"])}
    else:
        for k in ("node_start", "edge_start", "edge_dst"):      # the graph dump holds every node whatever the threshold: what was modelled on it stays
            assert np.array_equal(g[k], base["g"][k]), k
        m = {k: base[k] for k in ("front", "frags", "sup", "n_ovf")}
        if "reads" in base:
            m["reads"] = base["reads"]
    w, pre = executor_paths(tmp, 0, u.k, u.iv, cov)
    assert pre == o["pre"]
    wm = WM.build(g, cov)
    n_pos = int(m["front"]["n_pos"])
    assert n_pos == int(wm["n_pos"]) == int(g["n_pos"])
    m.update(u=u, tmp=tmp, cov=cov, o=o, g=g, ref=bytes(g["pos_nuc"]), wm=wm, node=PM.id_nodes(g, cov, wm), n_pos=n_pos, n_ids=int(wm["n_ids"]),
             side_xpos=np.ascontiguousarray(wm["side_xpos"], np.uint32), w=w)
    m["tables"] = {"own": w, "interleaved": LKU.links_tables(n_pos)["interleaved"]}
    m["windows"] = {"whole": (0, n_pos), "middle": (n_pos // 3 // 64 * 64 + 7, min(n_pos, 2 * n_pos // 3 + 13))}
    return m


def reads_of(m):
    if "reads" not in m:
        m["reads"] = ERM.reads(m["front"], m["g"], m["u"].k, m["u"].iv)
    return m["reads"]


def where(field, got, want):
    """the field and the first index at which two values of it differ"""
    if (np.isscalar(got) or np.isscalar(want)) and not isinstance(got, (bytes, bytearray)):
        return "%s = %s, expected %s" % (field, got, want)
    a = np.frombuffer(bytes(got), np.uint8) if isinstance(got, (bytes, bytearray)) else np.asarray(got)
    b = np.frombuffer(bytes(want), np.uint8) if isinstance(want, (bytes, bytearray)) else np.asarray(want)
    a, b = a.astype(np.int64).reshape(-1), b.astype(np.int64).reshape(-1)
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    if len(d):
        return "%s[%d] = %d, expected %d" % (field, int(d[0]), int(a[d[0]]), int(b[d[0]]))
    return "%s has %d entries, expected %d" % (field, len(a), len(b))


def _by_field(fn):
    """a comparator of the models that returns the first field that differs -> one that also names the index"""
    def same(got, want):
        d = fn(got, want)
        return None if d is None else where(d, got[d], want[d])
    return same


def _table(got, want):
    x = UU.table_mismatch(got, want)
    return None if x is None else x[2]


def _mapped(got, want):
    x = _table(got, want[0])
    if x is not None:
        return x
    try:
        same_map(got["id_map"], want[1])
    except AssertionError:
        for f in ("n_pos", "n_ids") + tuple(UU.RUNS):
            if not np.array_equal(got["id_map"][f], want[1][f]):
                return "id_map: " + where(f, got["id_map"][f], want[1][f])
        raise
    return None


def _support(got, want):
    x = _table(got, want[0])
    if x is not None:
        return x
    return None if got["link_support"].tolist() == want[1] else where("link_support", got["link_support"], want[1])


def _edge_support(got, want):
    """got: (Unit.edge_support(), Unit.graph()) — the counts are in agx_unit_graph's numbering, which check_counts holds them against"""
    got, graph = got
    try:
        check_counts(got, graph, want)
    except AssertionError:
        for f in ("edge_start", "edge_dst", "edge_cnt"):
            if not np.array_equal(got[f], want[f]):
                return where(f, got[f], want[f])
        for f in ("edge_start", "edge_dst", "n_nodes", "n_edges"):
            if not np.array_equal(got[f], graph[f]):
                return "against agx_unit_graph: " + where(f, got[f], graph[f])
        for f in ("n_events", "n_contributions"):
            if int(got[f]) != int(want[f]):
                return where(f, int(got[f]), int(want[f]))
        raise
    return None


def _edge_reads(got, want):
    try:
        edge_reads_same(got, want)      # (the per-kind file's: the values and the types of the binding's arrays)
    except AssertionError as x:
        d = ERM.same(got, want)
        return where(d, got[d], want[d]) if d is not None else "the type of %s" % x
    return None


def _links(got, want):
    x = _by_field(LM.same)(got, want)
    if x is None and not LM.identity(got):
        return "the classes do not add up to the fragments"
    return x


def _bubbles(got, want):
    return BM.mismatch(got, want)


def link_support_want(m, t, lo, hi, cov):
    """the support of every link of a model's table over [lo, hi) at cov: tail node -> head node in tests/edge_support_model.py's counts"""
    g = m["g"]
    t = {k: np.asarray(v) for k, v in t.items() if k != "seq"}
    tails = tails_of(g, t, lo, hi, cov)
    heads = g["node_start"].astype(np.int64)[t["head_pos"].astype(np.int64)] + t["head_var"].astype(np.int64)
    want = [ESM.edge_support_of(m["sup"], int(tails[a]), int(heads[b])) for a, b in zip(t["link_from"].tolist(), t["link_to"].tolist())]
    assert None not in want, (lo, hi, cov)
    return want


class Kind:
    def __init__(self, name, asks, call, want, same):
        """asks: the labels of the argument sets; call(e, i), want(i): the engine's and the model's answer to set i; same(got, want) of one answer"""
        self.name, self.asks, self._call, self._want, self._same, self._made = name, list(asks), call, want, same, None

    def call(self, e):
        return [self._call(e, i) for i in range(len(self.asks))]

    def want(self):
        if self._made is None:
            self._made = [self._want(i) for i in range(len(self.asks))]
        return self._made

    def same(self, got, want):
        if len(got) != len(want):
            return "%s: %d answers, expected %d" % (self.name, len(got), len(want))
        for label, a, b in zip(self.asks, got, want):
            x = self._same(a, b)
            if x is not None:
                return "%s, %s: %s" % (self.name, label, x)
        return None


def table(m, support=True):
    """kind -> Kind for a modelled unit.  support=False: the unit has no edge counters — the evidence is asked without min_support and modelled without steps, the bubbles
    without their rows' support; the kinds of NEEDS_SUPPORT are in the table all the same (the session tests ask them and expect the refusal)."""
    if ("table", support) in m:      # (made once per unit: so are its answers)
        return m[("table", support)]
    g, ref, cov, n_pos = m["g"], m["ref"], m["cov"], m["n_pos"]
    wins = [("whole", m["windows"]["whole"], cov), ("middle", m["windows"]["middle"], cov), ("middle at 0", m["windows"]["middle"], 0)]
    labels = [w[0] for w in wins]
    tabs = list(m["tables"].items())
    region = lambda i: R.region_unitigs(g, wins[i][1][0], wins[i][1][1], wins[i][2], ref)
    out = {}

    def add(name, asks, call, want, same):
        out[name] = Kind(name, asks, call, want, same)

    add("unitigs", ["whole export"], lambda e, i: e.unitigs(), lambda i: M.unitigs(g, cov, ref), _table)
    add("region", labels, lambda e, i: e.unitigs(region=wins[i][1], min_coverage=wins[i][2]), region, _table)

    def mapped_want(i):
        (lo, hi), c = wins[i][1], wins[i][2]
        mu = PM.id_map(g, cov, lo, hi, c, ref, m["wm"])[0]
        assert UU.table_mismatch(mu, region(i)) is None
        return mu, mu["id_map"]
    add("mapped", labels, lambda e, i: e.unitigs(region=wins[i][1], min_coverage=wins[i][2], id_map=True), mapped_want, _mapped)

    def support_want(i):
        t = region(i)
        return t, link_support_want(m, t, wins[i][1][0], wins[i][1][1], wins[i][2])
    add("support", labels, lambda e, i: e.unitigs(region=wins[i][1], min_coverage=wins[i][2], edge_support=True), support_want, _support)
    add("edge_support", ["counts"], lambda e, i: (e.edge_support(), e.graph()), lambda i: m["sup"], _edge_support)

    reads = [("whole", m["windows"]["whole"], ERM.ALL), ("middle <= 2", m["windows"]["middle"], 2)]
    add("edge_reads", [r[0] for r in reads], lambda e, i: e.edge_reads(reads[i][1], reads[i][2]),
        lambda i: ERM.table(reads_of(m), g, reads[i][1][0], reads[i][1][1], reads[i][2]), _edge_reads)

    ts = evidence_thresholds(g, cov)
    ev = [(tabs[0], ts[1] if support else (cov, 0)), (tabs[1], ts[2])]      # the build's coverage with the default support; a depth above every node's: every base weak
    add("evidence", ["%s at %s" % (t[0], th) for t, th in ev], lambda e, i: e.walk_evidence(ev[i][0][1], ev[i][1][0], ev[i][1][1], tracks=True),
        lambda i: EM.evidence(g, cov, ev[i][0][1], m["sup"] if support else None, ev[i][1][0], ev[i][1][1], wm=m["wm"], node=m["node"]),
        _by_field(lambda a, b: EM.same(a, b, tracks=True)))

    spans = [("whole", m["windows"]["whole"]), ("middle", m["windows"]["middle"])]
    add("pair_span", [s[0] for s in spans], lambda e, i: e.pair_span(spans[i][1]), lambda i: SM.pair_span(m["front"], spans[i][1], m["frags"]), _by_field(SM.same_span))

    def based(i):
        key = "based_" + tabs[i][0]
        if key not in m:
            m[key] = SM.bases(m["front"], m["side_xpos"], tabs[i][1], m["frags"])
        return m[key]

    def min_span(i):      # the median span under the unit's own stretches, one above every span under the hand table: every base thin
        return span_thresholds(m, based(i))[2 + i]
    add("walk_span", ["%s" % t[0] for t in tabs], lambda e, i: e.walk_span(tabs[i][1], min_span(i), tracks=True),
        lambda i: SM.walk_span(m["front"], m["side_xpos"], tabs[i][1], min_span(i), frags=m["frags"], based=based(i)), _by_field(lambda a, b: SM.same(a, b, tracks=True)))
    add("mate_links", ["%s" % t[0] for t in tabs], lambda e, i: e.mate_links(tabs[i][1], 1),
        lambda i: LM.mate_links(m["frags"], n_pos, m["side_xpos"], tabs[i][1], 1), _links)

    bub = [("whole" + (" with support" if support else ""), m["windows"]["whole"], cov, support), ("middle at 0", m["windows"]["middle"], 0, False)]

    def bubbles_want(i):
        (lo, hi), c = bub[i][1], bub[i][2]
        t = R.region_unitigs(g, lo, hi, c, ref)
        return BM.bubbles(t, link_support_want(m, t, lo, hi, c) if bub[i][3] else None)
    add("bubbles", [b[0] for b in bub], lambda e, i: e.bubbles(region=bub[i][1], min_coverage=bub[i][2], edge_support=bub[i][3]), bubbles_want, _bubbles)
    if not support:      # (what does not depend on the counters is asked and answered as on a unit with them)
        full = table(m)
        out.update({k: full[k] for k in KINDS if k not in ("evidence", "bubbles")})
    assert tuple(out) == KINDS
    m[("table", support)] = out
    return out
