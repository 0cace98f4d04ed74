"""The region model (tests/unitig_region_model.py) on hand-made graphs: every case states the segments and links it expects, written out by hand.
The GPU tests compare agx_unit_unitigs_region with this model, so what the model means is pinned here, without a device."""
import numpy as np

import unitig_model as M
import unitig_region_model as R

A, C, G, T = (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0)
NOVOTE = (0, 0, 0, 0, 0)


def S(name, seq, kc, pe):
    return b"S\t%s\t%s\tLN:i:%d\tKC:i:%d\tpe:i:%d\n" % (name, seq, len(seq), kc, pe)


def L(a, b):
    return b"L\t%s\t+\t%s\t+\t0M\n" % (a, b)


def chain():
    """Eight positions, one node each, coverage 5, i -> i + 1: one unitig ACGTACGT."""
    nodes = [(None, 5, v) for v in (A, C, G, T, A, C, G, T)]
    return M.graph_from_lists([1] * 8, nodes, [(i, i + 1) for i in range(7)]), b"N" * 8


def branch():
    """pos 0: a; pos 1: x (variant 0, isolated, coverage 2), b (variant 1); pos 2: e; pos 3: c (no votes: the reference base).  a -> b, a -> c, b -> e."""
    nodes = [(None, 5, A), (None, 2, C), (None, 5, G), (None, 5, T), (None, 5, NOVOTE)]
    return M.graph_from_lists([1, 2, 1, 1], nodes, [(0, 2), (0, 4), (2, 3)]), b"ACGT"


def pruned():
    """pos 0: a; pos 1: b (variant 0), p (variant 1, coverage 1: pruned at 5); pos 2: c (contig 7, coverage 0).  a -> b, a -> p, b -> c."""
    nodes = [(None, 5, A), (None, 5, C), (None, 1, G), (7, 0, T)]
    return M.graph_from_lists([1, 2, 1], nodes, [(0, 1), (0, 2), (1, 3)]), b"NNN"


def test_a_window_cuts_a_unitig_in_two_places():
    g, ref = chain()
    assert M.unit_gfa(g, 1, ref, 0) == S(b"u0_0_0", b"ACGTACGT", 40, 7)
    # the middle piece is one segment, named after its first node inside the window
    assert R.region_gfa(g, 2, 6, 1, ref, 0) == S(b"u0_2_0", b"GTAC", 20, 5)
    assert R.region_gfa(g, 0, 3, 1, ref, 0) == S(b"u0_0_0", b"ACG", 15, 2)
    assert R.region_gfa(g, 5, 8, 1, ref, 0) == S(b"u0_5_0", b"CGT", 15, 7)


def test_a_branch_whose_one_arm_lies_outside_becomes_internal():
    g, ref = branch()
    whole = S(b"u3_0_0", b"A", 5, 0) + S(b"u3_1_0", b"C", 2, 1) + S(b"u3_1_1", b"GT", 10, 2) + S(b"u3_3_0", b"T", 5, 3) + \
        L(b"u3_0_0", b"u3_1_1") + L(b"u3_0_0", b"u3_3_0")
    assert M.unit_gfa(g, 1, ref, 3) == whole
    assert R.region_gfa(g, 0, 4, 1, ref, 3) == whole
    # c (position 3) is outside: a's only edge left is a -> b, which joins a to b and e; no link crosses the border
    assert R.region_gfa(g, 0, 3, 1, ref, 3) == S(b"u3_0_0", b"AGT", 15, 2) + S(b"u3_1_0", b"C", 2, 1)
    # a is outside: b keeps its name, variant 1 of ALL of position 1's variants, also where x is pruned
    assert R.region_gfa(g, 1, 4, 1, ref, 3) == S(b"u3_1_0", b"C", 2, 1) + S(b"u3_1_1", b"GT", 10, 2) + S(b"u3_3_0", b"T", 5, 3)
    assert R.region_gfa(g, 1, 4, 3, ref, 3) == S(b"u3_1_1", b"GT", 10, 2) + S(b"u3_3_0", b"T", 5, 3)


def test_a_threshold_that_revives_a_pruned_node_splits_a_unitig():
    g, ref = pruned()
    assert M.unit_gfa(g, 5, ref, 0) == S(b"u0_0_0", b"ACT", 10, 2)
    assert R.region_gfa(g, 0, 3, 5, ref, 0) == S(b"u0_0_0", b"ACT", 10, 2)
    for cov in (0, 1):
        assert R.region_gfa(g, 0, 3, cov, ref, 0) == S(b"u0_0_0", b"A", 5, 0) + S(b"u0_1_0", b"CT", 5, 2) + S(b"u0_1_1", b"G", 1, 1) + \
            L(b"u0_0_0", b"u0_1_0") + L(b"u0_0_0", b"u0_1_1")
    # a stricter cut: only the contig's node survives
    assert R.region_gfa(g, 0, 3, 1 << 30, ref, 0) == S(b"u0_2_0", b"T", 0, 2)
    assert R.region_gfa(g, 0, 2, 1 << 30, ref, 0) == b""


def test_a_window_of_one_position():
    g, ref = branch()
    assert R.region_gfa(g, 1, 2, 1, ref, 0) == S(b"u0_1_0", b"C", 2, 1) + S(b"u0_1_1", b"G", 5, 1)
    assert R.region_gfa(g, 3, 4, 1, ref, 0) == S(b"u0_3_0", b"T", 5, 3)


def test_an_empty_window():
    g, ref = branch()
    for at in (0, 2, 4):
        u = R.region_unitigs(g, at, at, 1, ref)
        assert len(u["head_pos"]) == 0 and len(u["link_from"]) == 0 and u["seq"] == b"" and u["seq_off"].tolist() == [0]
        assert R.region_gfa(g, at, at, 1, ref, 0) == b""


def test_the_graph_dump_is_left_as_it_was():
    g, ref = branch()
    key, cnt = g["node_key"].copy(), g["node_cnt"].copy()
    R.region_unitigs(g, 1, 2, 1, ref)
    assert np.array_equal(g["node_key"], key) and np.array_equal(g["node_cnt"], cnt)
