"""agx_bubbles_tsv (host only) field by field: names, positions, k, the six comma lists, `*` for a direct branch's name and bases, `.` for the support lists of a table
without support, no header line, and the tables it refuses."""
import numpy as np
import pytest

import aligngraph_amd as A
import bubbles_model as BM
import bubbles_units as BU


def table(support=True, max_nodes=None):
    t, sup = BU.hand_table()
    return A.unitigs_bubbles(t, sup if support else None, max_nodes)


def test_every_field():
    text = A.bubbles_tsv(table(), 7)
    assert text == BU.HAND_TSV
    lines = text.decode().split("\n")
    assert lines[-1] == "" and len(lines) == 3, "one line per bubble, each ended, no header line"
    f = lines[0].split("\t")
    assert len(f) == 11
    assert f[0] == "u7_0_0" and f[1] == "u7_300_1", "source and sink, the S lines' names"
    assert (f[2], f[3], f[4]) == ("2", "300", "3"), "the source's last position, the sink's head position, k"
    assert f[5].split(",") == ["u7_100_1", "u7_200_0", "*"], "a direct branch has no name"
    assert f[6].split(",") == ["2", "5", "0"] and f[7].split(",") == ["11", "21", "0"]
    assert f[8].split(",") == ["1000", "1001", "1002"] and f[9].split(",") == ["1003", "1004", "1002"], "a direct branch: one link, twice"
    assert f[10].split(",") == ["CG", "GTACG", "*"], "a direct branch has no bases"
    assert all(len(l.split("\t")[k].split(",")) == int(l.split("\t")[4]) for l in lines[:-1] for k in (5, 6, 7, 8, 9, 10))


def test_without_support_and_the_unit_number():
    lines = A.bubbles_tsv(table(support=False), 0).decode().splitlines()
    assert [l.split("\t")[8:10] for l in lines] == [[".", "."]] * 2
    assert lines[1].split("\t") == ["u0_300_1", "u0_600_0", "303", "600", "2", "u0_400_0,u0_500_1", "1,1", "41,51", ".", ".", "A,C"]
    assert A.bubbles_tsv(table(), 12).startswith(b"u12_0_0\tu12_300_1\t")


def test_the_models_text_and_empty_tables():
    t, sup = BU.hand_table()
    for mx in (None, BU.HAND_LONGEST - 1, 0):
        for s in (sup, None):
            assert A.bubbles_tsv(A.unitigs_bubbles(t, s, mx), 5) == BM.tsv(BM.bubbles(t, s, mx), 5)
    assert A.bubbles_tsv(table(max_nodes=0), 1) == b""


def test_large_numbers():
    b = table()
    b["br_cov"] = b["br_cov"].copy()
    b["br_cov"][0] = (1 << 40) + 5
    b["src_last"] = np.array([0xFFFFFFFE, 303], "uint32")
    f = A.bubbles_tsv(b, 0).decode().splitlines()[0].split("\t")
    assert f[2] == "4294967294" and f[7].split(",")[0] == "1099511627781"


def test_inconsistent_tables_are_refused():
    for field, value in (("br_off", [0, 6, 5]), ("br_off", [1, 3, 5]), ("br_seq_off", [0, 2, 7, 7, 8, 10]), ("br_seq_off", [0, 3, 7, 7, 8, 9]), ("br_nodes", [2, 5, 1, 1, 1])):
        b = table()
        b[field] = np.array(value, b[field].dtype)
        with pytest.raises(A.AgxError):
            A.bubbles_tsv(b, 0)
    b = table()
    b["br_pos"] = b["br_pos"][:-1]
    with pytest.raises(A.AgxError):
        A.bubbles_tsv(b, 0)
    with pytest.raises(A.AgxError):
        A.bubbles_tsv(table(), -1)
