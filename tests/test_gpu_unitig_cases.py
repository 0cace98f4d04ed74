"""The unitig export on the MI355X (-m gpu) on the hand-made units of tests/unitig_units.py, whose arms tests/test_unitig_cases.py asserts on the CPU: per case one unit,
built once per module with kept counts, kept paths and edge support.  Every named window and threshold of the region form against tests/unitig_region_model.py array
by array and as GFA text; the id map against tests/path_model.py; the links' support against tests/edge_support_model.py; the whole export against
tests/unitig_model.py, against the region form over every position, and again after every reprune the case names; the windows forwards, backwards and with a whole
export and a whole-window export at threshold 0 between each two (the reverse map holds whatever the last export left in it); and at the end finish() against the oracle.
Every comparison is exact.  A failure names the case, the window, the threshold, the first differing field and index, and the lane, block and piece of that node in the
piece model: that says which kernel to open.  What each case's widest window holds, and the durations on an MI355X, are in profiles/unitig_cases_gpu.txt."""
import contextlib
import os

import numpy as np
import pytest

import edge_support_model as ESM
import harness as H
import lean_units as LU
import path_model as PM
import unitig_model as M
import unitig_region_model as R
import unitig_units as UU
import walk_model as WM
import walk_units as WU
from hostsim import sim
from test_gpu_paths import same_map

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in UU.cases()}
KEYS = ("initial", "pre", "extended")
CHUNK = 45              # windows per test of the order check: five exports per window


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


class Made:
    """One case: its files, the oracle's run at the build's coverage, the piece models, the expected tables (each made once, never changed) and the built unit."""

    def __init__(self, agx, case, tmp, stack):
        self.case, self.tmp = case, tmp
        self.o = H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True)
        self.g = self.o["graph"]
        self.ctx = UU.Ctx(case, self.g)
        self.n, self.ref = self.ctx.n_pos, self.ctx.ref
        self._want, self._whole = {}, {}
        self.u = stack.enter_context(agx.Unit(k=LU.K, insert_variation=case.iv, coverage=case.coverage, keep_counts=True, keep_paths=True, edge_support=True))
        self.u.load_files(tmp, 0)
        self.u.upload()
        self.u.build()

    def want(self, w):
        if w not in self._want:
            t = R.region_unitigs(self.g, w[0], w[1], w[2], self.ref)
            self._want[w] = (t, M.gfa_text(t, 0))
        return self._want[w]

    def whole(self, cov):
        if cov not in self._whole:
            self._whole[cov] = M.unit_gfa(self.g, cov, self.ref, 0)
        return self._whole[cov]

    def check(self, w, t):
        x = UU.export_mismatch(self.case, self.ctx, w, t, self.want(w)[0])
        assert x is None, x


@pytest.fixture(scope="module")
def made(agx, built, tmp_path_factory):
    out = {}
    with contextlib.ExitStack() as stack:
        def get(name):
            if name not in out:
                out[name] = Made(agx, CASES[name], WU.write_unit(CASES[name].unit, str(tmp_path_factory.mktemp(name))), stack)
            return out[name]
        yield get


def export(m, w):
    return m.u.unitigs(region=(w[0], w[1]), min_coverage=w[2])


def text(m, w):
    return m.u.gfa(0, region=(w[0], w[1]), min_coverage=w[2])


@pytest.mark.parametrize("name", list(CASES))
def test_region_windows(made, name):
    m = made(name)
    assert m.u.stats()["n_pos"] == m.n
    for w in m.case.windows:
        t = export(m, w)
        m.check(w, t)
        got = text(m, w)
        assert got == m.want(w)[1], "%s: GFA text of window [%d, %d) at threshold %d (the table is the model's)" % (name, w[0], w[1], w[2])
        assert (got == b"") == (w in m.case.empty), (name, w)
    w = m.ctx.widest()
    P, t = m.ctx.pm(w), m.want(w)[0]
    print("%s: %d windows; widest [%d, %d) at threshold %d: kept %d, np %d, rounds %d, segments %d, links %d"
          % (name, len(m.case.windows), w[0], w[1], w[2], P.kept, P.np, P.rounds, len(t["head_pos"]), len(t["link_from"])))


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.maps])
def test_id_map(made, name):
    m = made(name)
    wm = WM.build(m.g, m.case.coverage)
    for w in m.case.maps:
        t = m.u.unitigs(region=(w[0], w[1]), min_coverage=w[2], id_map=True)
        mu = PM.id_map(m.g, m.case.coverage, w[0], w[1], w[2], m.ref, wm)[0]
        m.check(w, t)
        got, want = t["id_map"], mu["id_map"]
        assert (got["n_pos"], got["n_ids"]) == (want["n_pos"], want["n_ids"]), (name, w)
        for f in UU.RUNS:
            a, b = got[f].astype(np.int64), want[f].astype(np.int64)
            i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None if len(a) == len(b) else min(len(a), len(b)))
            assert i is None, "%s: id map of window [%d, %d) at threshold %d (n_main %d): %s differs at run %d of %d / %d: got %s, expected %s" % (
                name, w[0], w[1], w[2], w[1] - w[0], f, i, len(a), len(b), a[i:i + 1].tolist(), b[i:i + 1].tolist())
        same_map(got, want)
        UU.check_map_shapes(m.case, w, got, wm["side_xpos"])


def tail_id(P, g):
    last = P.chains[g][-1]
    return int(P.starts[last] + P.p_len[last] - 1)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.support])
def test_link_support(made, name):
    m = made(name)
    case = m.case
    front = sim.run(m.tmp, 0, LU.K, case.iv, case.coverage, front=True)["front"]
    sup = ESM.support(front, m.g, LU.K, case.iv)
    links = 0
    for w in case.windows:
        t = m.u.unitigs(region=(w[0], w[1]), min_coverage=w[2], edge_support=True)
        m.check(w, t)
        P = m.ctx.pm(w)
        head = [int(P.node[h]) for h in P.heads]                                          # canonical node of every segment's head and tail, from the piece model
        tail = [int(P.node[tail_id(P, g)]) for g in range(len(P.chains))]
        want = [ESM.edge_support_of(sup, tail[a], head[b]) for a, b in zip(t["link_from"].tolist(), t["link_to"].tolist())]
        assert None not in want, (name, w)
        got = t["link_support"].tolist()
        i = next((i for i in range(len(want)) if got[i] != want[i]), None) if len(got) == len(want) else min(len(got), len(want))
        assert i is None, "%s: window [%d, %d) at threshold %d: link_support[%d] = %s, expected %s (of %d / %d); its tail: %s" % (
            name, w[0], w[1], w[2], i, got[i:i + 1], want[i:i + 1], len(got), len(want),
            UU.where(P, tail_id(P, int(t["link_from"][i]))) if i < len(want) else "-")
        links += len(want)
    assert links > 100


@pytest.mark.parametrize("name", list(CASES))
def test_whole_export(made, name):
    m = made(name)
    cov = m.case.coverage
    first = m.u.gfa(0)
    assert first == m.whole(cov), "%s: the whole export at the build's coverage %d" % (name, cov)
    assert first == m.u.gfa(0, region=(0, m.n), min_coverage=cov), name
    assert first.count(b"S\t") > 0
    try:
        for c in m.case.reprune:
            m.u.reprune(c)
            got = m.u.gfa(0)
            assert got == m.whole(c), "%s: the whole export after a reprune to %d" % (name, c)
            assert got == m.u.gfa(0, region=(0, m.n), min_coverage=c), (name, c)
            assert m.u.gfa(0, region=(0, m.n), min_coverage=cov) == first, (name, c)      # an explicit threshold is served as before
    finally:
        m.u.reprune(cov)
    assert m.u.gfa(0) == first, "%s: the whole export after the reprune back to %d" % (name, cov)
    texts = {m.whole(c) for c in (cov,) + m.case.reprune}
    assert len(texts) == 1 + len(m.case.reprune), "%s: two thresholds ask the same question" % name


ORDER = [(n, part) for n, c in CASES.items() for part in range((len(c.windows) + CHUNK - 1) // CHUNK)]


@pytest.mark.parametrize("name,part", ORDER, ids=["%s-%d" % x for x in ORDER])
def test_order_of_exports(made, name, part):
    """Small windows after large ones, high thresholds after low ones, region exports after whole ones: every result is the first one for its window."""
    m = made(name)
    wins = m.case.windows[part * CHUNK:(part + 1) * CHUNK]
    first = {}
    for w in wins:
        first[w] = text(m, w)
        assert first[w] == m.want(w)[1], "%s: window [%d, %d) at threshold %d, forwards" % (name, w[0], w[1], w[2])
    for w in reversed(wins):
        assert text(m, w) == first[w], "%s: window [%d, %d) at threshold %d, backwards" % (name, w[0], w[1], w[2])
    whole, low = m.u.gfa(0), m.u.gfa(0, region=(0, m.n), min_coverage=0)
    for w in wins:
        assert m.u.gfa(0) == whole and m.u.gfa(0, region=(0, m.n), min_coverage=0) == low, (name, w)
        got = text(m, w)
        if got != first[w]:
            m.check(w, export(m, w))
        assert got == first[w], "%s: window [%d, %d) at threshold %d, behind a whole export and a whole window at threshold 0" % (name, w[0], w[1], w[2])


@pytest.mark.parametrize("name", list(CASES))
def test_finish_after_the_exports(made, name):
    """The last test of every case: after whatever exports and reprunes the tests above ran on the unit, the walk's three outputs are the oracle's."""
    m = made(name)
    w = m.case.windows[-1]
    before = text(m, w)
    assert before == m.want(w)[1]
    out = m.u.finish()
    for key in KEYS:
        assert out[key] == m.o[key], "%s: %s" % (name, key)
