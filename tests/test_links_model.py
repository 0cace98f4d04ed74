"""The mate-links model (tests/links_model.py) on one hand-made front of nine hits on forty positions and three records whose answers are written out here (CPU only).

Side ids 40 and 41 stand on positions 2 and 3.
  record 0   main ids 10 .. 19
  record 1   side ids 40, 41 (positions 2, 3: it lies left of record 0 through them), then main ids 19 .. 29 — position 19 lies under both records: record 0 owns it,
             record 1's base there is shadowed
  record 2   no graph base

  hit   mates                      fragment    own[f_lo]  own[f_hi]   class
  1     [12 .. 15]  [22 .. 25]     [12, 25]    0          1           link (0, 1)
  2     [19 .. 21]  [26 .. 28]     [19, 28]    0          1           link (0, 1): f_lo on the shared position
  3     [10 .. 11]  [3 .. 4]       [3, 11]     1          0           link (1, 0): the b mate lies left, on the side id's position
  4     [21 .. 23]  [25 .. 27]     [21, 27]    1          1           inside record 1
  5     [28 .. 29]  [33 .. 34]     [28, 34]    1          none        open to the right, on record 1
  6     [5 .. 6]    [13 .. 14]     [5, 14]     none       0           open to the left, on record 0
  7     [6 .. 7]    [7 .. 8]       [6, 8]      none       none        unowned
  8     [15 .. 20]  [36 .. 41]     [15, 39]    0          none        f_hi clamped to n_pos - 1; open to the right, on record 0
  9     as hit 1, skipped          none
"""
import numpy as np

import links_model as LM
import path_model as PM
import span_model as SM
from span_units import hand_front

N = LM.NONE
N_POS = 40
SIDE_XPOS = np.array([2, 3], np.uint32)
RECORDS = PM.stretches([(10, [(10, 19, 0, 0)]), (13, [(40, 41, 0, 0), (19, 29, 2, 0)]), (5, [])])


def front():
    return hand_front(N_POS, [dict(a=12, b=22, len=4), dict(a=19, b=26, len=3), dict(a=10, b=3, len=2), dict(a=21, b=25, len=3), dict(a=28, b=33, len=2), dict(a=5, b=13, len=2),
                              dict(a=6, b=7, len=2), dict(a=15, b=36, len=6), dict(a=12, b=22, len=4, skip=True)])


def test_fragments_are_the_span_models():
    lo, hi, kept, outside = SM.fragments(front())
    assert list(zip(lo.tolist(), hi.tolist())) == [(12, 25), (19, 28), (3, 11), (21, 27), (28, 34), (5, 14), (6, 8), (15, 39)] and (kept, outside) == (8, 0)


def test_owners():
    own, n_owned, n_shadowed = LM.owners(N_POS, SIDE_XPOS, RECORDS)
    assert own == [N, N, 1, 1] + [N] * 6 + [0] * 10 + [1] * 10 + [N] * 10
    assert (n_owned, n_shadowed) == (22, 1)
    assert LM.base_positions(N_POS, SIDE_XPOS, RECORDS)[10:13] == [(1, 2), (1, 3), (1, 19)]


def test_classes_and_links():
    l = LM.mate_links(SM.fragments(front()), N_POS, SIDE_XPOS, RECORDS, 1)
    assert {k: l[k] for k in LM.TOTALS} == dict(n_kept=8, n_outside=0, n_fragments=8, n_unowned=1, n_inside=1, n_open=3, n_link_pairs=3, n_links_all=2, n_owned=22, n_shadowed=1)
    assert LM.identity(l)
    assert l["rec_inside"].tolist() == [0, 1, 0] and l["rec_open_left"].tolist() == [1, 0, 0] and l["rec_open_right"].tolist() == [1, 1, 0]
    assert l["rec_links_out"].tolist() == [2, 1, 0] and l["rec_links_in"].tolist() == [1, 2, 0]
    assert [l[k].tolist() for k in LM.LINK_KEYS] == [[0, 1], [1, 0], [2, 1], [24, 9], [12, 3], [19, 3], [25, 11], [28, 11]]
    assert l["len_sum"].dtype == np.uint64 and l["a"].dtype == np.uint32


def test_threshold_cuts_the_table_only():
    frags = SM.fragments(front())
    one, zero, two, three = (LM.mate_links(frags, N_POS, SIDE_XPOS, RECORDS, t) for t in (1, 0, 2, 3))
    assert LM.same(zero, one) is None
    assert [two[k].tolist() for k in LM.LINK_KEYS] == [[0], [1], [2], [24], [12], [19], [25], [28]] and len(three["a"]) == 0
    for l in (two, three):
        assert all(int(l[k]) == int(one[k]) for k in LM.TOTALS) and all(np.array_equal(l[k], one[k]) for k in LM.REC_KEYS)


def test_text():
    l = LM.mate_links(SM.fragments(front()), N_POS, SIDE_XPOS, RECORDS, 1)
    assert LM.tsv(l, 7) == b"p7_0\tp7_1\t2\t24\t12\t19\t25\t28\np7_1\tp7_0\t1\t9\t3\t3\t11\t11\n"
