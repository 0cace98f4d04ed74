"""agx_walk_span_bed on hand-made interval tables: the BED text spelled out (CPU only: the formatter needs no device), and agx_walk_evidence_bed, which shares its
formatter, still writing its own words."""
import ctypes

import numpy as np
import pytest

import aligngraph_amd as A
import span_model as SM

N = 0xFFFFFFFF


def table(rows, n_recs=8):
    e = {k: np.array([r[j] for r in rows], np.uint32) for j, k in enumerate(A.IV_SPAN)}
    e["rec_graph_bases"] = np.zeros(n_recs, np.uint64)
    return e


def test_lines_spelled_out():
    e = table([(0, 3, 3, 3, N), (1, 0, 2, 3, 1), (1, 7, 4294967294, 0, 0), (7, 10, 11, N, N)])
    assert A.span_bed(e, 12) == (b"p12_0\t3\t4\tthin\t0\t+\tpm:i:3\tjm:i:.\n"
                                 b"p12_1\t0\t3\tthin\t0\t+\tpm:i:3\tjm:i:1\n"
                                 b"p12_1\t7\t4294967295\tthin\t0\t+\tpm:i:0\tjm:i:0\n"
                                 b"p12_7\t10\t12\tthin\t0\t+\tpm:i:.\tjm:i:.\n")
    assert A.span_bed(e, 12) == SM.bed(e, 12)
    w = {k: e[s] for k, s in zip(A.IV_EVIDENCE, A.IV_SPAN)}
    w["rec_graph_bases"] = e["rec_graph_bases"]
    assert A.evidence_bed(w, 12).splitlines()[1] == b"p12_1\t0\t3\tweak\t0\t+\tdm:i:3\tsm:i:1"      # the other user of the formatter


def test_the_models_text_on_random_tables():
    rng = np.random.default_rng(5)
    for seed in range(4):
        n = int(rng.integers(1, 200))
        first = rng.integers(0, 2 ** 31, n)
        rows = list(zip(rng.integers(0, 8, n).tolist(), first.tolist(), (first + rng.integers(0, 1000, n)).tolist(),
                        rng.choice([0, 1, 17, N - 1, N], n).tolist(), rng.choice([0, 2, N], n).tolist()))
        e = table(rows)
        text = A.span_bed(e, seed)
        assert text == SM.bed(e, seed) and text.count(b"\n") == n


def test_empty_and_inconsistent_tables():
    assert A.span_bed(table([]), 0) == b""
    with pytest.raises(A.AgxError) as x:      # an interval that ends in front of its first base
        A.span_bed(table([(0, 5, 4, 1, 1)]), 0)
    assert x.value.code == A.AGX_E_ARG
    with pytest.raises(A.AgxError) as x:      # a record the table does not have
        A.span_bed(table([(8, 0, 0, 1, 1)]), 0)
    assert x.value.code == A.AGX_E_ARG
    s = A.WalkSpan()
    s.n_recs, s.n_intervals = 1, 1            # intervals without arrays
    p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert A.lib().agx_walk_span_bed(ctypes.byref(s), 0, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG and not p.value and n.value == 0
    assert A.lib().agx_walk_span_bed(ctypes.byref(s), -1, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG
