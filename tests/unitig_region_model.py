"""numpy model of the region export (agx_unit_unitigs_region): the unitigs of the sub-graph of positions [lo, hi) whose nodes are alive at a
coverage of the caller's choice.

It shares nothing with the kernels: the canonical graph dump is copied, every node outside the window loses what could keep it alive (contig word NONE,
coverage -1, which no threshold >= 0 admits), and unitig_model.unitigs does the rest at the caller's threshold.  A dead node takes its edges with it, so an
edge across the window's border is dropped; positions, variant indexes and therefore segment names stay those of the whole unit.
"""
import numpy as np

import unitig_model as M


def region_graph(graph, lo, hi):
    """A copy of the graph dump in which only the nodes of positions [lo, hi) can be alive."""
    node_start = np.asarray(graph["node_start"], dtype=np.int64)
    n_pos = len(node_start) - 1
    assert 0 <= lo <= hi <= n_pos, "window [%d, %d) outside [0, %d)" % (lo, hi, n_pos)
    pos = np.repeat(np.arange(n_pos, dtype=np.int64), np.diff(node_start))
    outside = (pos < lo) | (pos >= hi)
    g = dict(graph)
    key = np.array(graph["node_key"], dtype=np.uint32).reshape(-1, 6).copy()
    cnt = np.array(graph["node_cnt"], dtype=np.int64).reshape(-1, 6).copy()
    key[outside, 0] = M.NONE
    cnt[outside, 0] = -1
    g["node_key"], g["node_cnt"] = key, cnt
    return g


def region_unitigs(graph, lo, hi, min_cov, ref):
    """Segments and links of the window: the model's side of Unit.unitigs(region=(lo, hi), min_coverage=min_cov)."""
    assert min_cov >= 0
    return M.unitigs(region_graph(graph, lo, hi), min_cov, ref)


def region_gfa(graph, lo, hi, min_cov, ref, unit):
    """Expected S and L lines of one unit's window."""
    return M.gfa_text(region_unitigs(graph, lo, hi, min_cov, ref), unit)
