"""agx_unitigs_gfa on hand-filled unitig tables: exact bytes (CPU only: the formatter needs no device)."""
import ctypes

import numpy as np
import pytest

import aligngraph_amd as A
from unitig_model import gfa_text


def table(n_segs=3, seed=0, links=True):
    rng = np.random.default_rng(seed)
    n_nodes = rng.integers(1, 40, n_segs).astype(np.uint64)
    off = np.zeros(n_segs + 1, np.uint64)
    off[1:] = np.cumsum(n_nodes)
    head_pos = np.sort(rng.choice(10 ** 6, n_segs, replace=False)).astype(np.uint32)
    lf = rng.integers(0, n_segs, 4 * n_segs) if links and n_segs else np.zeros(0, np.int64)
    lt = rng.integers(0, n_segs, len(lf))
    pairs = sorted(set(zip(lf.tolist(), lt.tolist())))
    return {"head_pos": head_pos, "head_var": rng.integers(0, 3, n_segs).astype(np.uint32), "n_nodes": n_nodes.astype(np.uint32),
            "last_pos": head_pos + n_nodes.astype(np.uint32), "coverage": rng.integers(0, 2 ** 40, n_segs).astype(np.uint64), "seq_off": off,
            "seq": bytes(rng.choice(list(b"ACGTN"), int(off[-1])).astype(np.uint8)),
            "link_from": np.array([a for a, _ in pairs], np.uint32), "link_to": np.array([b for _, b in pairs], np.uint32)}


def test_names_and_order():
    t = {"head_pos": np.array([5, 5, 9], np.uint32), "head_var": np.array([0, 2, 1], np.uint32), "n_nodes": np.array([2, 1, 3], np.uint32),
         "last_pos": np.array([6, 5, 11], np.uint32), "coverage": np.array([30, 0, 2 ** 33], np.uint64), "seq_off": np.array([0, 2, 3, 6], np.uint64),
         "seq": b"ACGTTN", "link_from": np.array([0, 1, 1], np.uint32), "link_to": np.array([2, 0, 2], np.uint32)}
    assert A.unitigs_gfa(t, 12) == (b"S\tu12_5_0\tAC\tLN:i:2\tKC:i:30\tpe:i:6\n"
                                    b"S\tu12_5_2\tG\tLN:i:1\tKC:i:0\tpe:i:5\n"
                                    b"S\tu12_9_1\tTTN\tLN:i:3\tKC:i:8589934592\tpe:i:11\n"
                                    b"L\tu12_5_0\t+\tu12_9_1\t+\t0M\n"
                                    b"L\tu12_5_2\t+\tu12_5_0\t+\t0M\n"
                                    b"L\tu12_5_2\t+\tu12_9_1\t+\t0M\n")


def test_random_tables_match_the_model_text():
    for seed in range(5):
        t = table(50, seed)
        assert A.unitigs_gfa(t, seed) == gfa_text(t, seed)


def test_offsets_beyond_4gb():
    # the table's offsets start 2^32 + 7 bases into its sequence: the struct's seq points that far in front of the bases it holds, so every offset
    # needs 64 bits (without 4 GB of bases)
    t = table(20, 3)
    bias = 2 ** 32 + 7
    want = A.unitigs_gfa(t, 0)
    s, keep = A._unitigs_struct(dict(t, seq_off=t["seq_off"] + np.uint64(bias)))
    assert s.seq > bias
    s.seq -= bias
    s.n_bases = int(t["seq_off"][-1]) + bias
    assert A._gfa_text(s, 0) == want
    assert keep


def test_empty_table():
    t = {k: np.zeros(0, np.uint32) for k in ("head_pos", "head_var", "n_nodes", "last_pos", "link_from", "link_to")}
    t.update(coverage=np.zeros(0, np.uint64), seq_off=np.zeros(1, np.uint64), seq=b"")
    assert A.unitigs_gfa(t, 0) == b""


def test_one_thread_and_many_give_the_same_text(monkeypatch):
    t = table(5000, 11)
    monkeypatch.setenv("AGX_GFA_THREADS", "1")
    one = A.unitigs_gfa(t, 4)
    for n in ("3", "16", "64"):
        monkeypatch.setenv("AGX_GFA_THREADS", n)
        assert A.unitigs_gfa(t, 4) == one
    assert one == gfa_text(t, 4)


def test_inconsistent_tables_are_refused():
    t = table(10, 5)
    for bad in (dict(link_to=np.full(len(t["link_to"]), 10, np.uint32)), dict(n_nodes=t["n_nodes"] + np.uint32(1)),
                dict(seq_off=t["seq_off"][::-1].copy())):
        with pytest.raises(A.AgxError) as e:
            A.unitigs_gfa(dict(t, **bad), 0)
        assert e.value.code == A.AGX_E_ARG
    assert ctypes.sizeof(A.Unitigs) == 88
