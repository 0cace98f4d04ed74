"""The evidence model (tests/evidence_model.py) on one hand-made graph of twelve nodes whose answers are written out here (CPU only).

  position     0    1    2        3    4    5    6    7         8     9
  nodes        n0 - n1 - n2 (v0)- n4 - n5 - n6 - n7 - n8 (v0) - n10 - n11        n1 -> n2, n1 -> n3; n2 -> n4, n3 -> n4; n7 -> n8, n7 -> n9; n8 -> n10, n9 -> n10
                       \\ n3 (v1)/                   \\ n9 (v1)/
  coverage     5    5    5, 4     3    2    6    6    8, 3      9     9          built at coverage 3: n5 is pruned, main id 4 has no node
  walk ids     0    1    2, 10    3    4    5    6    7, 11     8     9          (n_pos = 10: two side ids)
  support      0-1: 10, 1-2: 7, 1-3: 2, 2-4: 6, 3-4: 1, 4-5: 2, 5-6: 2, 6-7: 5, 7-8: 4, 7-9: 1, 8-10: 4, 9-10: 1, 10-11: 8
"""
import numpy as np

import evidence_model as EM
import path_model as PM
import unitig_model as M

N = EM.NONE
COV = 3
EDGES = {(0, 1): 10, (1, 2): 7, (1, 3): 2, (2, 4): 6, (3, 4): 1, (4, 5): 2, (5, 6): 2, (6, 7): 5, (7, 8): 4, (7, 9): 1, (8, 10): 4, (9, 10): 1, (10, 11): 8}


def graph():
    depth = [5, 5, 5, 4, 3, 2, 6, 6, 8, 3, 9, 9]
    nodes = [(None, d, (d, 0, 0, 0, 0) if i % 2 else (0, 0, d, 0, 0)) for i, d in enumerate(depth)]
    nodes[7] = (None, 6, (3, 4, 0, 0, 0))                    # a node whose votes are split: the largest counter is 4
    g = M.graph_from_lists([1, 1, 2, 1, 1, 1, 1, 2, 1, 1], nodes, sorted(EDGES))
    z = np.zeros(g["n_pos"], np.uint32)
    g.update({"pos_nuc": b"T" * 10, "chain_end": z, "cm_count": z, "hop_off": z, "hop_len": z, "hop_end": z, "hop_str": b""})
    return g


def support():
    pairs = sorted(EDGES)
    start = np.searchsorted(np.array([s for s, _ in pairs]), np.arange(13))
    return {"edge_start": start.astype(np.uint32), "edge_dst": np.array([d for _, d in pairs], np.uint32), "edge_cnt": np.array([EDGES[p] for p in pairs], np.uint32)}


# record 0: one stretch; 1: a side id, then joined onto main ids of which one has no node; 2: two stretches with a chain between them and a depth tie;
# 3: three one-base stretches, the last step names no edge (n10 -> n0); 4: a record without a stretch
RECORDS = PM.stretches([(8, [(0, 3, 0, 0)]), (9, [(10, 10, 0, 0), (3, 5, 1, 1)]), (20, [(5, 7, 0, 0), (8, 9, 10, 0)]), (6, [(11, 11, 0, 0), (8, 8, 1, 1), (0, 0, 2, 1)]), (5, [])])


def test_walk_ids():
    assert PM.id_nodes(graph(), COV).tolist() == [0, 1, 2, 4, -1, 6, 7, 8, 10, 11, 3, 9]


def test_tracks_and_totals():
    e = EM.evidence(graph(), COV, RECORDS, support())
    assert e["depth"].tolist() == [5, 5, 5, 3, 4, 3, N, 6, 6, 6, 8, 9, 9, 3, 9, 5]
    assert e["votes"].tolist() == [5, 5, 5, 3, 4, 3, N, 6, 6, 4, 8, 9, 9, 3, 9, 5]
    assert e["step"].tolist() == [10, 7, 6, N, 1, N, N, N, 5, 4, N, 8, N, 1, N, N]
    assert e["track_off"].tolist() == [0, 4, 5, 8, 11, 13, 14, 15, 16]
    assert (e["n_graph_bases"], e["n_steps"], e["n_steps_without_edge"]) == (16, 8, 1)


def test_record_summaries():
    e = EM.evidence(graph(), COV, RECORDS, support())
    assert e["rec_graph_bases"].tolist() == [4, 4, 5, 3, 0]
    assert e["rec_steps"].tolist() == [3, 1, 3, 1, 0]
    assert e["rec_depth_sum"].tolist() == [18, 13, 38, 17, 0]
    assert e["rec_depth_min"].tolist() == [3, 3, 6, 3, N] and e["rec_depth_min_at"].tolist() == [3, 1, 0, 0, 0]      # record 2: 6 at offsets 0 and 1, the smaller one
    assert e["rec_step_min"].tolist() == [6, 1, 4, 1, N] and e["rec_step_min_at"].tolist() == [2, 0, 1, 0, 0]


def intervals(e):
    return list(zip(*(e[k].tolist() for k in EM.IV_KEYS)))


def test_weak_intervals():
    g, s = graph(), support()
    assert intervals(EM.evidence(g, COV, RECORDS, s, 0, 0)) == [(1, 2, 2, N, N)]                                  # only the base without a node
    assert intervals(EM.evidence(g, COV, RECORDS, s, 4, 2)) == [(0, 3, 3, 3, N), (1, 0, 2, 3, 1), (3, 0, 0, 3, 1)]      # record 1: a weak step, a thin base, no node: one interval across the joined boundary
    assert intervals(EM.evidence(g, COV, RECORDS, s, 0, 5)) == [(1, 0, 0, 4, 1), (1, 2, 2, N, N), (2, 1, 1, 6, 4), (3, 0, 0, 3, 1)]
    # above every depth: every graph base is weak; intervals end at a chain (record 2) and at a record's end
    assert intervals(EM.evidence(g, COV, RECORDS, s, 10, 0)) == [(0, 0, 3, 3, 6), (1, 0, 3, 3, 1), (2, 0, 2, 6, 4), (2, 10, 11, 9, 8), (3, 0, 2, 3, 1)]


def test_without_counters_every_step_is_none():
    e = EM.evidence(graph(), COV, RECORDS, None, 4, 0)
    assert set(e["step"].tolist()) == {N} and (e["n_steps"], e["n_steps_without_edge"]) == (0, 0)
    assert intervals(e) == [(0, 3, 3, 3, N), (1, 1, 2, 3, N), (3, 0, 0, 3, N)]
    assert e["rec_step_min"].tolist() == [N] * 5 and e["rec_steps"].tolist() == [0] * 5


def test_tracks_of_a_record_range_and_bed():
    e = EM.evidence(graph(), COV, RECORDS, support(), 4, 2, records=(1, 3))
    assert e["track_off"].tolist() == [0, 1, 4, 7, 9] and e["depth"].tolist() == [4, 3, N, 6, 6, 6, 8, 9, 9] and e["step"].tolist() == [1, N, N, N, 5, 4, N, 8, N]
    assert EM.bed(e, 7) == b"p7_0\t3\t4\tweak\t0\t+\tdm:i:3\tsm:i:.\np7_1\t0\t3\tweak\t0\t+\tdm:i:3\tsm:i:1\np7_3\t0\t1\tweak\t0\t+\tdm:i:3\tsm:i:1\n"
