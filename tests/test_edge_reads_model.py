"""tests/edge_reads_model.py pinned: on one small unit the answer is written out by hand, and on every unit the other edge-reads tests use, the list behind every
edge is as long as tests/edge_support_model.py says the edge's support is — the two models share their route, so this only says that keeping the hit numbers lost or
doubled nothing.

The hand unit (k = 5, reads of 100 bases, every position one variant): hit 0 lies at 100, hit 1 at 150, hit 2 at 100 with three bases deleted behind its index 39.
A hit steps from the position of its index i to that of i + 1 for i < 95, so hit 0 names the edges x -> x + 1 for x in [100, 195), hit 1 for x in [150, 245), hit 2
for x in [100, 139) and [143, 198) and the edge 139 -> 143."""
import os

import numpy as np
import pytest

import edge_reads_model as ERM
import edge_support_model as ESM
import harness as H
import lean_units as LU
from hostsim import sim
from test_edge_support_cases import UNITS, modelled  # noqa: F401  (modelled: the module fixture)


def hand_unit():
    return LU.Unit(512, [LU.pair(100, 300), LU.pair(150, 350), LU.pair(100, 300, left_cigar="40M3D60M")])


def hand_answer():
    want = {}
    for h, spans in enumerate([[(100, 195)], [(150, 245)], [(100, 139), (143, 198)]]):
        for lo, hi in spans:
            for x in range(lo, hi):
                want.setdefault((x, x + 1), []).append(h)
    want[(139, 143)] = [2]
    return want


@pytest.fixture(scope="module")
def hand(built, tmp_path_factory):
    tmp = LU.write_unit(hand_unit(), str(tmp_path_factory.mktemp("edge_reads_hand")))
    g = H.run_oracle(tmp, 0, LU.K, LU.IV, 1, graph=True)["graph"]
    front = sim.run(tmp, 0, LU.K, LU.IV, 1, front=True)["front"]
    return g, front, ERM.reads(front, g, LU.K, LU.IV)


def test_hand_unit(hand):
    g, front, rd = hand
    assert len(front["dhit"]) == 3 and (np.diff(g["node_start"].astype(np.int64)) <= 1).all()
    got = {}
    for (s, d), hits in rd.items():
        (sp, dp), (sv, dv) = ERM.pos_var(g, [s, d])
        assert (int(sv), int(dv)) == (0, 0)
        got[(int(sp), int(dp))] = hits
    assert got == hand_answer()


def test_hand_table(hand):
    g, front, rd = hand
    t = ERM.table(rd, g)
    assert len(t["src_pos"]) == 146 and int(t["hit_off"][-1]) == len(t["hit"]) == 3 * 95      # 145 steps x -> x + 1 and the jump; three hits of 95 events
    at = t["src_pos"].tolist().index(139)
    assert (t["src_pos"][at:at + 2].tolist(), t["dst_pos"][at:at + 2].tolist(), t["support"][at:at + 2].tolist()) == ([139, 139], [140, 143], [1, 1])
    assert t["hit"][int(t["hit_off"][at]):int(t["hit_off"][at + 2])].tolist() == [0, 2]
    one = ERM.table(rd, g, 139, 144, 1)      # window [139, 144) at support 1: 139 -> 140 (hit 0), 139 -> 143 (hit 2), 140.., 141.., 142.. (hit 0); 143 -> 144 has two
    assert (one["src_pos"].tolist(), one["dst_pos"].tolist(), one["hit"].tolist()) == ([139, 139, 140, 141, 142], [140, 143, 141, 142, 143], [0, 2, 0, 0, 0])
    assert len(ERM.table(rd, g, 0, 512, 0)["src_pos"]) == 0 and len(ERM.table(rd, g, 200, 200)["src_pos"]) == 0
    assert ERM.table(rd, g, 150, 151, 3)["hit"].tolist() == [0, 1, 2]


@pytest.mark.parametrize("name", list(UNITS))
def test_list_lengths_are_the_support(modelled, name):
    u, tmp, g, front, model = modelled(name)
    rd = ERM.reads(front, g, u.k, u.iv)
    assert {e: len(h) for e, h in rd.items()} == model["pairs"]
    assert all(len(set(h)) == len(h) for h in rd.values()), "one hit names an edge in one event at most"
    t = ERM.table(rd, g)
    assert int(t["hit_off"][-1]) == model["n_contributions"] and len(t["support"]) == int(g["n_edges"])
