"""agx_unitigs_gfa_support on hand-made unitig tables: agx_unitigs_gfa's bytes with RC:i:<n> appended to every L line (CPU only: the formatter needs no device)."""
import ctypes
import re

import numpy as np
import pytest

import aligngraph_amd as A
from test_gfa_format import table


def test_tags_on_a_small_table():
    t = {"head_pos": np.array([5, 5, 9], np.uint32), "head_var": np.array([0, 2, 1], np.uint32), "n_nodes": np.array([2, 1, 3], np.uint32),
         "last_pos": np.array([6, 5, 11], np.uint32), "coverage": np.array([30, 0, 2 ** 33], np.uint64), "seq_off": np.array([0, 2, 3, 6], np.uint64),
         "seq": b"ACGTTN", "link_from": np.array([0, 1, 1], np.uint32), "link_to": np.array([2, 0, 2], np.uint32), "link_support": np.array([500, 1, 4294967295], np.uint32)}
    assert A.unitigs_gfa(t, 12, edge_support=True) == (b"S\tu12_5_0\tAC\tLN:i:2\tKC:i:30\tpe:i:6\n"
                                                       b"S\tu12_5_2\tG\tLN:i:1\tKC:i:0\tpe:i:5\n"
                                                       b"S\tu12_9_1\tTTN\tLN:i:3\tKC:i:8589934592\tpe:i:11\n"
                                                       b"L\tu12_5_0\t+\tu12_9_1\t+\t0M\tRC:i:500\n"
                                                       b"L\tu12_5_2\t+\tu12_5_0\t+\t0M\tRC:i:1\n"
                                                       b"L\tu12_5_2\t+\tu12_9_1\t+\t0M\tRC:i:4294967295\n")


@pytest.mark.parametrize("threads", ["1", "7"])
def test_stripped_of_the_tag_the_bytes_are_the_plain_export(monkeypatch, threads):
    monkeypatch.setenv("AGX_GFA_THREADS", threads)
    for seed in range(4):
        t = table(300, seed)
        sup = np.random.default_rng(seed).integers(0, 2 ** 32, len(t["link_from"])).astype(np.uint32)
        text = A.unitigs_gfa(dict(t, link_support=sup), seed, edge_support=True)
        assert re.sub(rb"\tRC:i:\d+\n", b"\n", text) == A.unitigs_gfa(t, seed)
        tags = [int(m) for m in re.findall(rb"^L\t.*\tRC:i:(\d+)$", text, re.M)]
        assert tags == sup.tolist() and len(tags) == text.count(b"\nL\t")
        assert b"RC:i:" not in b"".join(ln for ln in text.split(b"\n") if ln.startswith(b"S"))


def test_null_array_and_wrong_length_are_refused():
    t = table(10, 5)
    s, keep = A._unitigs_struct(t)
    p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert A.lib().agx_unitigs_gfa_support(ctypes.byref(s), None, 0, ctypes.byref(p), ctypes.byref(n)) == A.AGX_E_ARG
    assert not p.value and n.value == 0 and keep
    with pytest.raises(A.AgxError) as e:
        A.unitigs_gfa(dict(t, link_support=np.zeros(len(t["link_from"]) + 1, np.uint32)), 0, edge_support=True)
    assert e.value.code == A.AGX_E_ARG
    with pytest.raises(A.AgxError) as e:      # the table itself is still checked
        A.unitigs_gfa(dict(t, link_to=np.full(len(t["link_to"]), 10, np.uint32), link_support=np.zeros(len(t["link_from"]), np.uint32)), 0, edge_support=True)
    assert e.value.code == A.AGX_E_ARG


def test_empty_table_with_an_array():
    t = {k: np.zeros(0, np.uint32) for k in ("head_pos", "head_var", "n_nodes", "last_pos", "link_from", "link_to")}
    t.update(coverage=np.zeros(0, np.uint64), seq_off=np.zeros(1, np.uint64), seq=b"", link_support=np.zeros(0, np.uint32))
    s, keep = A._unitigs_struct(t)
    one = (ctypes.c_uint32 * 1)(0)
    p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    assert A.lib().agx_unitigs_gfa_support(ctypes.byref(s), one, 0, ctypes.byref(p), ctypes.byref(n)) == A.AGX_OK and n.value == 0 and keep
    A.lib().agx_text_free(p)
