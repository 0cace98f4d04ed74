"""agx_mate_links_tsv on hand-made link tables: the text spelled out (CPU only: the formatter needs no device)."""
import ctypes

import numpy as np
import pytest

import aligngraph_amd as A
import links_model as LM


def table(rows, n_recs=8):
    l = {k: np.array([r[j] for r in rows], np.uint64 if k == "len_sum" else np.uint32) for j, k in enumerate(A.LINK_LINKS)}
    l["rec_inside"] = np.zeros(n_recs, np.uint32)
    return l


def test_lines_spelled_out():
    l = table([(0, 1, 2, 24, 12, 19, 25, 28), (1, 0, 1, 9, 3, 3, 11, 11), (6, 7, 4294967295, 2 ** 63 + 5, 0, 4294967294, 1, 4294967294)])
    assert A.links_tsv(l, 12) == (b"p12_0\tp12_1\t2\t24\t12\t19\t25\t28\n"
                                  b"p12_1\tp12_0\t1\t9\t3\t3\t11\t11\n"
                                  b"p12_6\tp12_7\t4294967295\t9223372036854775813\t0\t4294967294\t1\t4294967294\n")
    assert A.links_tsv(l, 12) == LM.tsv(l, 12) and A.links_tsv(l) == LM.tsv(l, 0)
    assert A.LINK_LINKS == LM.LINK_KEYS and A.REC_LINKS == LM.REC_KEYS


def test_the_models_text_on_random_tables():
    rng = np.random.default_rng(7)
    for seed in range(4):
        n = int(rng.integers(1, 200))
        a = rng.integers(0, 8, n)
        lo = rng.integers(0, 2 ** 31, n)
        rows = list(zip(a.tolist(), ((a + rng.integers(1, 8, n)) % 8).tolist(), rng.integers(1, 2 ** 32, n).tolist(), rng.integers(1, 2 ** 62, n).tolist(),
                        lo.tolist(), (lo + rng.integers(0, 1000, n)).tolist(), (lo + 1000).tolist(), (lo + 2000).tolist()))
        l = table(rows)
        text = A.links_tsv(l, seed)
        assert text == LM.tsv(l, seed) and text.count(b"\n") == n and all(line.count(b"\t") == 7 for line in text.splitlines())


def test_empty_and_inconsistent_tables():
    assert A.links_tsv(table([]), 0) == b""
    for rows in ([(8, 0, 1, 1, 0, 0, 1, 1)], [(0, 8, 1, 1, 0, 0, 1, 1)], [(3, 3, 1, 1, 0, 0, 1, 1)]):      # a record the table does not have; a link of a record to itself
        with pytest.raises(A.AgxError) as x:
            A.links_tsv(table(rows), 0)
        assert x.value.code == A.AGX_E_ARG
    s = A.MateLinks()
    s.n_recs, s.n_links = 2, 1                # links without arrays
    p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert A.lib().agx_mate_links_tsv(ctypes.byref(s), 0, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG and not p.value and n.value == 0
    assert A.lib().agx_mate_links_tsv(ctypes.byref(s), -1, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG
