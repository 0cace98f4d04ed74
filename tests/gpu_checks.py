"""Comparisons that more than one GPU test file makes: the downloaded walk graph against tests/walk_model.py (tests/test_gpu_walk_graph.py,
tests/test_gpu_sweep_passes.py) and the edge-support counts against tests/edge_support_model.py (tests/test_gpu_edge_support.py, tests/test_gpu_sweep_passes.py)."""
import numpy as np

import walk_model as WM


def check_walk(o, dumps, out, cov, executor=None, sparse_min=False):
    m = WM.build(o["graph"], cov, sparse_min=sparse_min)
    for w in dumps:
        assert WM.mismatch(m, w) is None
        if executor is not None:
            assert WM.same_bits(executor, w) is None
    for key in ("initial", "pre", "extended"):
        assert out[key] == o[key], key
    assert out["stats"]["n_walk_ids"] == m["n_ids"] and out["stats"]["n_special"] == m["n_special"]
    return m


def check_counts(got, graph, model):
    assert np.array_equal(got["edge_start"], graph["edge_start"]) and np.array_equal(got["edge_dst"], graph["edge_dst"])
    assert np.array_equal(got["edge_start"], model["edge_start"]) and np.array_equal(got["edge_dst"], model["edge_dst"])
    assert got["n_nodes"] == graph["n_nodes"] and got["n_edges"] == graph["n_edges"]
    assert np.array_equal(got["edge_cnt"], model["edge_cnt"])
    assert got["n_events"] == model["n_events"] and got["n_contributions"] == model["n_contributions"]
    assert (got["edge_cnt"] >= 1).all()
