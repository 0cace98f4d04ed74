"""tests/bubbles_model.py pinned by hand on the written-out table of tests/bubbles_units.py: one fork of each class, a three-way bubble, a bubble whose sink is the next
bubble's source, a direct branch, and max_nodes at one below, at and one above the longest branch."""
import bubbles_model as BM
import bubbles_units as BU


def rows(b):
    return {f: b[f] for f in BM.PER_BUBBLE + BM.PER_BRANCH + (BM.SUPPORT if b["has_support"] else ()) + ("seq",)}


def test_every_fork_has_its_class():
    t, _ = BU.hand_table()
    assert BM.classes(t) == BU.HAND_CLASSES
    assert set(c for c, _ in BU.HAND_CLASSES.values()) == {"bubble", "tip", "nested", "sinks_differ", "sink_shared"}


def test_totals_and_rows_with_support():
    t, sup = BU.hand_table()
    b = BM.bubbles(t, sup)
    assert {f: b[f] for f in BM.TOTALS} == BU.HAND_TOTALS
    assert rows(b) == BU.HAND_ALL
    assert b["br_off"][1] - b["br_off"][0] == 3, "a three-way bubble"
    assert b["sink_pos"][0] == b["src_pos"][1] and b["sink_var"][0] == b["src_var"][1], "the first bubble's sink is the second one's source"
    assert b["br_sup_in"][2] == b["br_sup_out"][2], "a direct branch is one link"


def test_rows_without_support():
    t, _ = BU.hand_table()
    b = BM.bubbles(t)
    assert not b["has_support"] and "br_sup_in" not in b
    assert rows(b) == {f: v for f, v in BU.HAND_ALL.items() if f not in BM.SUPPORT}


def test_max_nodes_around_the_longest_branch():
    t, sup = BU.hand_table()
    n = BU.HAND_LONGEST
    short, at, above = BM.bubbles(t, sup, n - 1), BM.bubbles(t, sup, n), BM.bubbles(t, sup, n + 1)
    assert rows(short) == BU.HAND_SHORT and rows(at) == BU.HAND_ALL and rows(above) == BU.HAND_ALL
    assert rows(BM.bubbles(t, sup, 0)) == {f: ([0] if f in ("br_off", "br_seq_off") else b"" if f == "seq" else []) for f in rows(at)}
    for b in (short, at, above):
        assert {f: b[f] for f in BM.TOTALS} == BU.HAND_TOTALS, "the totals do not depend on max_nodes"


def test_text():
    t, sup = BU.hand_table()
    assert BM.tsv(BM.bubbles(t, sup), 7) == BU.HAND_TSV
    plain = BM.tsv(BM.bubbles(t), 7).decode().splitlines()
    assert [l.split("\t")[8:10] for l in plain] == [[".", "."]] * 2
    assert BM.tsv(BM.bubbles(t, sup, 0), 7) == b""


def test_mismatch_names_the_first_difference():
    t, sup = BU.hand_table()
    want = BM.bubbles(t, sup)
    assert BM.mismatch(BM.bubbles(t, sup), want) is None
    other = BM.bubbles(t, sup)
    other["br_cov"][3] += 1
    assert BM.mismatch(other, want) == "br_cov[3] = 42, expected 41"
