"""agx_edge_reads_tsv on hand-made tables: the TSV text spelled out (CPU only: the formatter needs no device).  DESIGN.md section 15 says one hit names an edge in one
event at most, so no table of the engine lists a hit twice behind an edge and none is made up here; the formatter itself prints whatever list it is given."""
import ctypes

import numpy as np
import pytest

import aligngraph_amd as A

N = 0xFFFFFFFF


def table(rows):
    """rows: (src_pos, src_var, dst_pos, dst_var, support, [hits])"""
    r = {k: np.array([row[j] for row in rows], np.uint32) for j, k in enumerate(A.EDGE_READS_EDGE)}
    r["hit_off"] = np.concatenate([[0], np.cumsum([len(row[5]) for row in rows])]).astype(np.uint64)
    r["hit"] = np.array([h for row in rows for h in row[5]], np.uint32)
    return r


def test_empty_result():
    assert A.edge_reads_tsv(table([]), 0) == b""
    assert A.edge_reads_tsv(table([]), 7) == b""


def test_one_edge():
    assert A.edge_reads_tsv(table([(139, 0, 143, 0, 1, [2])]), 0) == b"0\t139\t0\t143\t0\t1\t2\n"


def test_lines_spelled_out():
    r = table([(5, 0, 6, 1, 3, [0, 7, 4294967294]), (5, 1, 6, 0, 1, [12]), (4294967294, 1023, 4294967295, 65535, 2, [3, 4])])
    assert A.edge_reads_tsv(r, 12) == (b"12\t5\t0\t6\t1\t3\t0,7,4294967294\n"
                                      b"12\t5\t1\t6\t0\t1\t12\n"
                                      b"12\t4294967294\t1023\t4294967295\t65535\t2\t3,4\n")


def test_text_against_plain_python_on_random_tables():
    rng = np.random.default_rng(5)
    for seed in range(4):
        n = int(rng.integers(1, 120))
        rows = []
        for _ in range(n):
            hits = sorted(set(rng.integers(0, 2 ** 32, int(rng.integers(1, 9))).tolist()))
            rows.append(tuple(rng.integers(0, 2 ** 32, 4).tolist()) + (len(hits), hits))
        want = "".join("%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % ((seed,) + row[:5] + (",".join(map(str, row[5])),)) for row in rows).encode()
        assert A.edge_reads_tsv(table(rows), seed) == want


def test_inconsistent_tables():
    r = table([(1, 0, 2, 0, 1, [5]), (2, 0, 3, 0, 1, [6])])
    r["hit_off"] = np.array([0, 2, 1], np.uint64)      # offsets that do not rise to n_hits
    with pytest.raises(A.AgxError) as x:
        A.edge_reads_tsv(r, 0)
    assert x.value.code == A.AGX_E_ARG
    r["hit_off"] = np.array([0, 1], np.uint64)          # one offset short
    with pytest.raises(A.AgxError) as x:
        A.edge_reads_tsv(r, 0)
    assert x.value.code == A.AGX_E_ARG
    s = A.EdgeReads()
    s.n_edges = 1                                      # edges without arrays
    p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert A.lib().agx_edge_reads_tsv(ctypes.byref(s), 0, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG and not p.value and n.value == 0
    assert A.lib().agx_edge_reads_tsv(ctypes.byref(s), -1, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG
