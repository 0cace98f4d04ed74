"""The path model (tests/path_model.py) on one hand-made graph whose answers are written out here: a bubble, a path that starts in the middle of a unitig, a
conti-mer chain between two stretches, a node that is dead at the export's threshold, and windows that cut the records (CPU only).

  position     0    1    2        3    4    5
  nodes        n0 - n1 - n2 (v0)- n4 - n5 - n6          n1 -> n2, n1 -> n3; n2 -> n4, n3 -> n4
                       \\ n3 (v1)/
  coverage     5    5    5, 5     3    5    5          built at coverage 3: every node has a walk id
  walk ids     0    1    2, 6     3    4    5          (n_pos = 6: the second variant of position 2 is the one side id)
"""
import numpy as np

import path_model as PM
import unitig_model as M

REF = b"TTTTTT"
COV = 3


def graph():
    votes = {"A": (9, 0, 0, 0, 0), "C": (0, 9, 0, 0, 0), "G": (0, 0, 9, 0, 0), "T": (0, 0, 0, 9, 0)}
    nodes = [(None, 5, votes["A"]), (None, 5, votes["C"]), (None, 5, votes["G"]), (None, 5, votes["T"]), (None, 3, votes["A"]), (None, 5, votes["C"]), (None, 5, votes["G"])]
    g = M.graph_from_lists([1, 1, 2, 1, 1, 1], nodes, [(0, 1), (1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (5, 6)])
    n_pos = g["n_pos"]
    z = np.zeros(n_pos, np.uint32)
    g.update({"pos_nuc": REF, "chain_end": z, "cm_count": z, "hop_off": z, "hop_len": z, "hop_end": z, "hop_str": b""})      # (what walk_model.build reads besides the tables: no conti-mers)
    return g


# record 0: the first unitig; 1: through the bubble's first branch; 2: the bubble's second branch (the side id), then over an edge onto the main ids; 3: begins in the
# middle of the last unitig; 4: two stretches with a seven-base conti-mer chain between them.  Every record ends in a four-base k-mer tail, which is no stretch.
RECORDS = PM.stretches([(6, [(0, 1, 0, 0)]), (8, [(2, 5, 0, 0)]), (8, [(6, 6, 0, 0), (3, 5, 1, 1)]), (6, [(4, 5, 0, 0)]), (16, [(0, 1, 0, 0), (3, 5, 9, 0)])])


def check(lo, hi, min_cov, heads, lengths, runs, text):
    g = graph()
    u, e_seg, e_rank = PM.id_map(g, COV, lo, hi, min_cov, REF)
    assert list(zip(u["head_pos"].tolist(), u["head_var"].tolist())) == heads and u["n_nodes"].tolist() == lengths
    m = u["id_map"]
    assert (m["n_pos"], m["n_ids"]) == (6, 7)
    assert list(zip(m["id_first"].tolist(), m["id_last"].tolist(), m["seg"].tolist(), m["rank_first"].tolist())) == runs
    assert PM.paths_gfa(u, e_seg, e_rank, RECORDS, 0) == text


def test_walk_ids_of_the_hand_made_graph():
    assert PM.id_nodes(graph(), COV).tolist() == [0, 1, 2, 4, 5, 6, 3]
    assert PM.id_nodes(graph(), 5).tolist() == [0, 1, 2, -1, 5, 6, 3]      # built at 5 the node of position 3 is pruned: its main id has no node


def test_bubble_mid_unitig_start_and_chain_break():
    check(0, 6, 3, [(0, 0), (2, 0), (2, 1), (3, 0)], [2, 1, 1, 3], [(0, 1, 0, 0), (2, 2, 1, 0), (3, 5, 3, 0), (6, 6, 2, 0)],
          b"P\tp0_0_0\tu0_0_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_1_0\tu0_2_0+,u0_3_0+\t*\tln:i:4\tfs:i:0\tls:i:2\n"
          b"P\tp0_2_0\tu0_2_1+,u0_3_0+\t*\tln:i:4\tfs:i:0\tls:i:2\n"
          b"P\tp0_3_0\tu0_3_0+\t*\tln:i:2\tfs:i:1\tls:i:2\n"
          b"P\tp0_4_0\tu0_0_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_4_9\tu0_3_0+\t*\tln:i:3\tfs:i:0\tls:i:2\n")


def test_a_node_dead_at_the_threshold_breaks_the_paths():
    check(0, 6, 5, [(0, 0), (2, 0), (2, 1), (4, 0)], [2, 1, 1, 2], [(0, 1, 0, 0), (2, 2, 1, 0), (4, 5, 3, 0), (6, 6, 2, 0)],
          b"P\tp0_0_0\tu0_0_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_1_0\tu0_2_0+\t*\tln:i:1\tfs:i:0\tls:i:0\n"
          b"P\tp0_1_2\tu0_4_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_2_0\tu0_2_1+\t*\tln:i:1\tfs:i:0\tls:i:0\n"
          b"P\tp0_2_2\tu0_4_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_3_0\tu0_4_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_4_0\tu0_0_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_4_10\tu0_4_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n")


def test_window_borders_cut_the_paths():
    check(0, 3, 3, [(0, 0), (2, 0), (2, 1)], [2, 1, 1], [(0, 1, 0, 0), (2, 2, 1, 0), (6, 6, 2, 0)],
          b"P\tp0_0_0\tu0_0_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n"
          b"P\tp0_1_0\tu0_2_0+\t*\tln:i:1\tfs:i:0\tls:i:0\n"
          b"P\tp0_2_0\tu0_2_1+\t*\tln:i:1\tfs:i:0\tls:i:0\n"
          b"P\tp0_4_0\tu0_0_0+\t*\tln:i:2\tfs:i:0\tls:i:1\n")
    check(3, 6, 3, [(3, 0)], [3], [(3, 5, 0, 0)],
          b"P\tp0_1_1\tu0_3_0+\t*\tln:i:3\tfs:i:0\tls:i:2\n"
          b"P\tp0_2_1\tu0_3_0+\t*\tln:i:3\tfs:i:0\tls:i:2\n"
          b"P\tp0_3_0\tu0_3_0+\t*\tln:i:2\tfs:i:1\tls:i:2\n"
          b"P\tp0_4_9\tu0_3_0+\t*\tln:i:3\tfs:i:0\tls:i:2\n")
    check(2, 2, 3, [], [], [], b"")                                 # an empty window
    check(3, 4, 0, [(3, 0)], [1], [(3, 3, 0, 0)],                  # one position, nothing pruned
          b"P\tp0_1_1\tu0_3_0+\t*\tln:i:1\tfs:i:0\tls:i:0\n"
          b"P\tp0_2_1\tu0_3_0+\t*\tln:i:1\tfs:i:0\tls:i:0\n"
          b"P\tp0_4_9\tu0_3_0+\t*\tln:i:1\tfs:i:0\tls:i:0\n")


def test_a_step_that_is_no_edge_of_the_export_is_refused():
    import pytest
    g = graph()
    u, e_seg, e_rank = PM.id_map(g, COV, 0, 6, 3, REF)
    with pytest.raises(AssertionError):
        PM.paths(u, e_seg, e_rank, PM.stretches([(6, [(0, 1, 0, 0), (4, 5, 2, 1)])]))      # "joined" from id 1 to id 4: there is no such link
