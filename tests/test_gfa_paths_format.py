"""agx_unitigs_paths_gfa on hand-made tables: exact bytes against the path model's text, and AGX_E_ARG for tables that do not agree (CPU only: the formatter
needs no device)."""
import numpy as np
import pytest

import aligngraph_amd as A
import path_model as PM
from test_path_model import COV, RECORDS, REF, graph


@pytest.mark.parametrize("lo,hi,min_cov", [(0, 6, 3), (0, 6, 5), (0, 3, 3), (3, 6, 3), (2, 2, 3), (3, 4, 0), (1, 5, 4)])
def test_text_is_the_models(lo, hi, min_cov):
    u, e_seg, e_rank = PM.id_map(graph(), COV, lo, hi, min_cov, REF)
    want = PM.paths_gfa(u, e_seg, e_rank, RECORDS, 7)
    assert A.gfa_paths(u, RECORDS, 7) == want
    assert (want != b"") == (hi > lo)
    assert want.replace(b"p7_", b"p0_").replace(b"u7_", b"u0_") == A.gfa_paths(u, RECORDS, 0)


def test_no_records_and_no_runs():
    u, _, _ = PM.id_map(graph(), COV, 0, 6, 3, REF)
    assert A.gfa_paths(u, PM.stretches([]), 0) == b""
    assert A.gfa_paths(u, PM.stretches([(4, [])]), 0) == b""              # a record of chain bases only
    empty = dict(u, id_map=dict(u["id_map"], **{k: np.zeros(0, np.uint32) for k in ("id_first", "id_last", "seg", "rank_first")}))
    assert A.gfa_paths(empty, RECORDS, 0) == b""


def table():
    """Two segments: A (four nodes, at position 10) and B (two nodes, at position 14), one link A -> B.  Main ids 0..3 are A's nodes, 4..5 are B's."""
    t = {"head_pos": np.array([10, 14], np.uint32), "head_var": np.array([0, 0], np.uint32), "n_nodes": np.array([4, 2], np.uint32), "last_pos": np.array([13, 15], np.uint32),
         "coverage": np.array([40, 20], np.uint64), "seq_off": np.array([0, 4, 6], np.uint64), "seq": b"ACGTAC", "link_from": np.array([0], np.uint32), "link_to": np.array([1], np.uint32)}
    t["id_map"] = {"n_pos": 20, "n_ids": 22, "id_first": np.array([0, 4], np.uint32), "id_last": np.array([3, 5], np.uint32), "seg": np.array([0, 1], np.uint32),
                   "rank_first": np.array([0, 0], np.uint32)}
    return t


def with_map(t, **kw):
    return dict(t, id_map=dict(t["id_map"], **{k: np.array(v, np.uint32) for k, v in kw.items()}))


def refused(t, w):
    with pytest.raises(A.AgxError) as e:
        A.gfa_paths(t, w, 0)
    assert e.value.code == A.AGX_E_ARG


def test_inconsistent_tables_are_refused():
    w = PM.stretches([(10, [(1, 5, 0, 0)])])
    t = table()
    assert A.gfa_paths(t, w, 3) == b"P\tp3_0_0\tu3_10_0+,u3_14_0+\t*\tln:i:5\tfs:i:1\tls:i:1\n"
    # a rank gap: id 2 would be A's last node right behind id 1 = A's second
    refused(with_map(t, id_first=[0, 2, 4], id_last=[1, 2, 5], seg=[0, 0, 1], rank_first=[0, 3, 0]), w)
    # the step from A's last node onto B without that link in the table
    refused(dict(t, link_from=np.zeros(0, np.uint32), link_to=np.zeros(0, np.uint32)), w)
    refused(dict(t, link_from=np.array([1], np.uint32), link_to=np.array([0], np.uint32)), w)
    # onto B's second node
    refused(with_map(t, id_first=[0, 4], id_last=[3, 4], seg=[0, 1], rank_first=[0, 1]), w)
    # runs out of order, overlapping, beyond their segment, naming no segment, across the main ids' end
    refused(with_map(t, id_first=[4, 0], id_last=[5, 3], seg=[1, 0], rank_first=[0, 0]), w)
    refused(with_map(t, id_first=[0, 3], id_last=[3, 5], seg=[0, 1], rank_first=[0, 0]), w)
    refused(with_map(t, id_first=[0, 4], id_last=[3, 6], seg=[0, 1], rank_first=[0, 0]), w)
    refused(with_map(t, id_first=[0, 4], id_last=[3, 5], seg=[0, 2], rank_first=[0, 0]), w)
    refused(with_map(t, id_first=[0, 19], id_last=[3, 20], seg=[0, 1], rank_first=[0, 0]), w)
    # stretches that do not describe a record: beyond the record, a first stretch that is joined, `joined` that disagrees with the offsets, ids beyond the unit
    refused(t, PM.stretches([(4, [(1, 5, 0, 0)])]))
    refused(t, PM.stretches([(10, [(1, 5, 0, 1)])]))
    refused(t, PM.stretches([(10, [(1, 2, 0, 0), (3, 5, 2, 0)])]))
    refused(t, PM.stretches([(10, [(1, 2, 0, 0), (3, 5, 3, 1)])]))
    refused(t, PM.stretches([(10, [(1, 2, 0, 0), (3, 5, 1, 0)])]))
    refused(t, PM.stretches([(10, [(20, 22, 0, 0)])]))
    # and the same records cut where the tables allow it
    assert A.gfa_paths(t, PM.stretches([(10, [(1, 2, 0, 0), (3, 5, 2, 1)])]), 0) == b"P\tp0_0_0\tu0_10_0+,u0_14_0+\t*\tln:i:5\tfs:i:1\tls:i:1\n"
    assert A.gfa_paths(t, PM.stretches([(12, [(1, 2, 0, 0), (3, 5, 4, 0)])]), 0) == (b"P\tp0_0_0\tu0_10_0+\t*\tln:i:2\tfs:i:1\tls:i:2\n"
                                                                                   b"P\tp0_0_4\tu0_10_0+,u0_14_0+\t*\tln:i:3\tfs:i:3\tls:i:1\n")
