"""tests/edge_support_model.py pinned with answers written out by hand, on tiny lean_units.Unit's: the model is what the shim and the kernel are measured against
(tests/test_edge_support_cases.py, tests/test_gpu_edge_support.py), so its own numbers are stated here without it."""
import numpy as np
import pytest

import edge_support_model as ESM
import edge_units as EU
import harness as H
import lean_units as LU
from hostsim import sim
from lean_units import K, L, Unit, pair

NONE = ESM.NONE


@pytest.fixture(scope="module")
def run(built, tmp_path_factory):
    def go(name, unit, iv=LU.IV):
        tmp = LU.write_unit(unit, str(tmp_path_factory.mktemp(name)))
        g = H.run_oracle(tmp, 0, K, iv, 1, graph=True)["graph"]
        front = sim.run(tmp, 0, K, iv, 1, front=True)["front"]
        return g, front, ESM.support(front, g, K, iv)
    return go


def node(g, x, v=0):
    assert g["node_start"][x] + v < g["node_start"][x + 1], "no variant %d at %d" % (v, x)
    return int(g["node_start"][x]) + v


def variants_at(g, x):
    return int(g["node_start"][x + 1]) - int(g["node_start"][x])


def test_identical_pairs_every_edge_of_the_stretch_has_support_n(run):
    n, x0 = 7, 1000
    g, front, s = run("pile", Unit(4096, [pair(x0, x0 + 400)] * n))
    # one read: sources are the indices 0 .. L - k - 1, the last one steps onto index L - k (jstar), nothing lies beyond it
    assert s["n_events"] == n * (L - K) and s["n_contributions"] == n * (L - K)
    assert int(g["n_edges"]) == L - K
    for i in range(L - K):
        assert ESM.edge_support_of(s, node(g, x0 + i), node(g, x0 + i + 1)) == n
    assert variants_at(g, x0 + L - K) == 1 and variants_at(g, x0 + L - K + 1) == 0
    assert int(s["edge_start"][node(g, x0 + L - K) + 1]) - int(s["edge_start"][node(g, x0 + L - K)]) == 0      # the last position is no source
    E = ESM.events(front, K)
    assert E[:, 0].max() == x0 + L - K - 1 and E[:, 1].max() == x0 + L - K
    assert s["off_graph"] == 0 and sorted(s["pairs"].values()) == [n] * (L - K)


def test_branch_edges_carry_two_and_one(run):
    """edge_units.variants(x, 2) with 2 + 1 reads: two reads whose mates lie SEP apart make two variants at every position they cover; a third read joins the first.
    The two strands of the stretch carry 2 and 1 on every edge and no event crosses between them."""
    x = 2048 + 30
    g, front, s = run("strands", Unit(4096, EU.variants(x, 2) + [EU.end_at(x, x + EU.OFF)]))
    for p in range(x - (L - K), x):
        assert variants_at(g, p) == 2 and variants_at(g, p + 1) == 2
        assert ESM.edge_support_of(s, node(g, p, 0), node(g, p + 1, 0)) == 2
        assert ESM.edge_support_of(s, node(g, p, 1), node(g, p + 1, 1)) == 1
        assert ESM.edge_support_of(s, node(g, p, 0), node(g, p + 1, 1)) is None and ESM.edge_support_of(s, node(g, p, 1), node(g, p + 1, 0)) is None
    assert s["off_graph"] == 0 and s["n_events"] == 3 * (L - K) == s["n_contributions"]


def test_a_real_branch_point(run):
    """insertVariation 0 (variants 25 apart).  Three reads on one left alignment; one of them has a 30-base deletion in its other mate behind index 49: up to x + 49 the
    three are one variant, from x + 50 on the third read is a variant of its own.  Two events step from x + 49 into variant 0 and one into variant 1."""
    x = 1024
    g, front, s = run("branch", Unit(4096, [pair(x, x + 400)] * 2 + [pair(x, x + 400, other_cigar="50M30D50M")]), iv=0)
    assert variants_at(g, x + 49) == 1 and variants_at(g, x + 50) == 2
    assert ESM.edge_support_of(s, node(g, x + 49), node(g, x + 50, 0)) == 2
    assert ESM.edge_support_of(s, node(g, x + 49), node(g, x + 50, 1)) == 1
    assert ESM.edge_support_of(s, node(g, x + 48), node(g, x + 49)) == 3
    assert ESM.edge_support_of(s, node(g, x + 50, 0), node(g, x + 51, 0)) == 2 and ESM.edge_support_of(s, node(g, x + 50, 1), node(g, x + 51, 1)) == 1
    assert s["off_graph"] == 0


def test_a_deletion_read_counts_on_the_jump_edge_only(run):
    x, d = 2048 + 20, 6
    g, front, s = run("dele", Unit(4096, EU.cover(x - 150, x + 200) + [EU.dele(x, [d])]))
    base = ESM.support(*run("dele_base", Unit(4096, EU.cover(x - 150, x + 200)))[1::-1], K, LU.IV)      # (front, graph) of the unit without the read
    assert ESM.edge_support_of(s, node(g, x), node(g, x + d + 1)) == 1
    for p in range(x, x + d + 1):      # x -> x + 1 and the skipped positions' edges: only the background's events
        got, was = ESM.edge_support_of(s, node(g, p), node(g, p + 1)), ESM.edge_support_of(base, node(g, p), node(g, p + 1))
        assert got == was and got >= 1, p
    assert s["n_events"] == base["n_events"] + (L - K)      # 40 + 60 aligned indices, the sources are those below L - k


def test_read_insertion_next_to_a_gap_makes_a_chain(run):
    """40M3I5D57M: index 39 lies on x + 39, indices 40..42 are inserted, index 43 lies on x + 45.  The event of index 39 steps to x + 40 without a mate position, the
    chain walks x + 40 .. x + 44 without mate positions at its sources, and its last event enters x + 45 with index 43's mate position."""
    x = 1024
    g, front, s = run("chain", Unit(4096, [pair(x, x + 400, left_cigar="40M3I5D57M")]))
    E = ESM.events(front, K)
    rows = {tuple(int(v) for v in r) for r in E}
    assert (x + 39, x + 40, x + 400 + 39, NONE) in rows
    for c in range(x + 40, x + 44):
        assert (c, c + 1, NONE, NONE) in rows
    assert (x + 44, x + 45, NONE, x + 400 + 43) in rows
    assert (x + 45, x + 46, x + 400 + 43, x + 400 + 44) in rows
    # 39 ordinary events in front (indices 0..38), index 39's, five chain events, then indices 43 .. L - k - 1
    assert len(E) == 39 + 1 + 5 + (L - K - 43)
    assert s["off_graph"] == 0 and (s["edge_cnt"] == 1).all() and s["n_contributions"] == len(E)
    for c in range(x + 39, x + 45):
        assert ESM.edge_support_of(s, node(g, c), node(g, c + 1)) == 1


def test_two_conti_mers_that_resolve_to_one_variant_count_once(run):
    """Two overlapping contigs on opposite strands: the positions under both carry two conti-mers, so an event there has two candidate keys at each end.  With one
    variant per position both keys resolve to it and the event names the edge once."""
    x = 1000
    g, front, s = run("twocm", Unit(4096, [pair(x, x + 400)] * 3, contigs=[(x - 400, x + 60, "+"), (x + 20, x + 600, "-")]))
    cms = front["cm_start"].astype(np.int64)
    both = [p for p in range(x + 25, x + 50) if cms[p + 1] - cms[p] == 2 and cms[p + 2] - cms[p + 1] == 2 and variants_at(g, p) == 1 and variants_at(g, p + 1) == 1]
    assert both, "no step between two positions with two conti-mers and one variant each"
    for p in both:
        assert ESM.edge_support_of(s, node(g, p), node(g, p + 1)) == 3
    assert s["off_graph"] == 0
