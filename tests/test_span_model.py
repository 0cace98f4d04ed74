"""The pair-span model (tests/span_model.py) on one hand-made front of five hits on thirty positions whose answers are written out here (CPU only).

  hit   mate a                       mate b           fragment
  A     runs [2 .. 5] and [8 .. 10]  [14 .. 20]       [2, 20]       a mate of two runs
  B     [10 .. 15]                   [13 .. 18]       [10, 18]      the mates overlap
  C     [20 .. 25]                   [24 .. 29+]      [20, 29]      mate b hangs over the last position: clamped, the fragment ends on it
  D     [17 .. 21]                   [5 .. 9]         [5, 21]       the b mate lies left
  E     [0 .. 29], skipped                            none

  position  0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28 29
  span      0  0  1  1  1  2  2  2  2  2  3  3  3  3  3  3  3  3  3  2  3  2  1  1  1  1  1  1  1  1
  ends                                                          B     A  D                       C
  cross     0  0  1  1  1  2  2  2  2  2  3  3  3  3  3  3  3  3  2  2  2  1  1  1  1  1  1  1  1  0

pairs(12, 22) = 0: A, B and D begin at or in front of 12, none of them reaches 22 — although cross[12] = 3 and no cross in between is below 1: the fragments relay.
pairs(19, 21) = 1 (D), cross[19] = cross[20] = 2.
"""
import numpy as np

import path_model as PM
import span_model as SM
from span_units import hand_front

N = SM.NONE
SPAN = [0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1]
CROSS = [0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 0]


def front():
    return hand_front(30, [dict(a=[(0, 2, 4), (4, 8, 3)], b=14, len=7), dict(a=10, b=13, len=6), dict(a=20, b=24, len=6), dict(a=17, b=5, len=5), dict(a=0, b=0, len=30, skip=True)])


# side ids 30 and 31 stand on positions 12 and 22.  record 0: one stretch; 1: a jump 12 -> 22 nobody spans; 2: the same jump through side ids, a step that is not
# forward (22 -> 19) and a jump one fragment spans (19 -> 21); 3: a record without a stretch
SIDE_XPOS = np.array([12, 22], np.uint32)
RECORDS = PM.stretches([(12, [(8, 13, 0, 0)]), (10, [(10, 12, 0, 0), (22, 24, 3, 1)]), (8, [(30, 30, 0, 0), (31, 31, 1, 1), (19, 19, 2, 1), (21, 21, 3, 1)]), (5, [])])


def test_fragments():
    lo, hi, kept, outside = SM.fragments(front())
    assert list(zip(lo.tolist(), hi.tolist())) == [(2, 20), (10, 18), (20, 29), (5, 21)] and (kept, outside) == (4, 0)


def test_span_and_cross():
    s = SM.pair_span(front())
    assert s["span"].tolist() == SPAN and s["cross"].tolist() == CROSS
    assert (s["n_kept"], s["n_fragments"], s["n_outside"], s["pos_lo"], s["pos_hi"]) == (4, 4, 0, 0, 30)
    w = SM.pair_span(front(), (19, 22))
    assert w["span"].tolist() == [2, 3, 2] and w["cross"].tolist() == [2, 2, 1] and w["n_fragments"] == 3 and w["n_kept"] == 4      # B ends on 18: it does not meet the window
    e = SM.pair_span(front(), (7, 7))
    assert len(e["span"]) == 0 and (e["n_fragments"], e["n_kept"]) == (0, 4)


def test_pairs():
    f = SM.fragments(front())
    assert SM.pairs(f, 12, 22) == 0 and CROSS[12] == 3 and min(CROSS[12:22]) == 1
    assert SM.pairs(f, 19, 21) == 1 and CROSS[19] == 2 and min(CROSS[19:21]) == 2
    assert all(SM.pairs(f, x, x + 1) == CROSS[x] for x in range(29))
    assert SM.pairs(f, 5, 20) == 2 and SM.pairs(f, 5, 21) == 1 and SM.pairs(f, 4, 21) == 0      # y == f_hi counts, y == f_hi + 1 does not; x == f_lo counts, x == f_lo - 1 does not


def test_an_outside_hit_and_a_mate_over_the_end():
    f = hand_front(30, [dict(a=30, b=40, len=5), dict(a=27, b=2, len=5)])
    lo, hi, kept, outside = SM.fragments(f)
    assert (lo.tolist(), hi.tolist(), kept, outside) == ([2], [29], 2, 1)


def test_tracks_and_totals():
    e = SM.walk_span(front(), SIDE_XPOS, RECORDS)
    assert e["pos"].tolist() == [8, 9, 10, 11, 12, 13, 10, 11, 12, 22, 23, 24, 12, 22, 19, 21]
    assert e["span"].tolist() == [2, 2, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 3, 1, 2, 2]
    assert e["step"].tolist() == [2, 2, 3, 3, 3, N, 3, 3, 0, 1, 1, N, 0, N, 1, N]
    assert e["track_off"].tolist() == [0, 6, 9, 12, 13, 14, 15, 16]
    assert (e["n_graph_bases"], e["n_steps"], e["n_jump_steps"], e["n_steps_not_forward"]) == (16, 12, 3, 1)


def test_record_summaries():
    e = SM.walk_span(front(), SIDE_XPOS, RECORDS)
    assert e["rec_graph_bases"].tolist() == [6, 6, 4, 0] and e["rec_steps"].tolist() == [5, 5, 2, 0] and e["rec_span_sum"].tolist() == [16, 12, 8, 0]
    assert e["rec_span_min"].tolist() == [2, 1, 1, N] and e["rec_span_min_at"].tolist() == [0, 3, 1, 0]      # record 0: 2 at offsets 0 and 1, the smaller one
    assert e["rec_step_min"].tolist() == [2, 0, 0, N] and e["rec_step_min_at"].tolist() == [0, 2, 0, 0]


def intervals(e):
    return list(zip(*(e[k].tolist() for k in SM.IV_KEYS)))


def test_thin_intervals():
    f = front()
    assert intervals(SM.walk_span(f, SIDE_XPOS, RECORDS, 0)) == []
    assert intervals(SM.walk_span(f, SIDE_XPOS, RECORDS, 1)) == [(1, 2, 2, 3, 0), (2, 0, 0, 3, 0)]      # only the jump nobody spans, at both of its bases
    assert intervals(SM.walk_span(f, SIDE_XPOS, RECORDS, 2)) == [(1, 2, 5, 1, 0), (2, 0, 2, 1, 0)]
    assert intervals(SM.walk_span(f, SIDE_XPOS, RECORDS, 3)) == [(0, 0, 1, 2, 2), (1, 2, 5, 1, 0), (2, 0, 3, 1, 0)]


def test_tracks_of_a_record_range_and_bed():
    e = SM.walk_span(front(), SIDE_XPOS, RECORDS, 2, records=(1, 3))
    assert e["track_off"].tolist() == [0, 3, 6, 7, 8, 9, 10] and e["pos"].tolist() == [10, 11, 12, 22, 23, 24, 12, 22, 19, 21] and e["step"].tolist() == [3, 3, 0, 1, 1, N, 0, N, 1, N]
    assert SM.bed(e, 7) == b"p7_1\t2\t6\tthin\t0\t+\tpm:i:1\tjm:i:0\np7_2\t0\t3\tthin\t0\t+\tpm:i:1\tjm:i:0\n"
    one = dict(e, iv_rec=[0], iv_first=[4], iv_last=[4], iv_span_min=[0], iv_step_min=[N])
    assert SM.bed(one, 0) == b"p0_0\t4\t5\tthin\t0\t+\tpm:i:0\tjm:i:.\n"
