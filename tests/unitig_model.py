"""numpy model of the unitig export: from a canonical graph dump (the oracle's, harness.run_oracle(..., graph=True), or a hand-made
one of the same form), the coverage threshold and the unit's reference bases, the exact GFA text agx_unitigs_gfa writes for the unit (S and L lines,
no header).

  alive node     contigID != -1 or coverage >= c                                  (AG:1904-1918)
  alive edge     u -> v between alive nodes, duplicates once
  internal edge  alive out-degree(u) = 1, alive in-degree(v) = 1, u != v
  unitig         a maximal path of internal edges, named by its head (position, variant); one base per node: max(A, C, G, T, N), ties A > C > G > T > N,
                 the reference base where all five are 0 (AG:1944-1952, 1995-2001)
"""
import os

import numpy as np

NONE = 0xFFFFFFFF
GFA_HEADER = b"H\tVN:Z:1.0\n"


def read_reference(tmp_dir, unit):
    """The bases of tmp/_genome.<unit>.fa (one record, any line length)."""
    out = []
    with open(os.path.join(tmp_dir, "_genome.%d.fa" % unit), "rb") as f:
        for line in f:
            if not line.startswith(b">"):
                out.append(line.rstrip(b"\r\n"))
    return b"".join(out)


def unitigs(graph, coverage, ref):
    """Segments and links as arrays: the model's side of Unit.unitigs()."""
    node_start = np.asarray(graph["node_start"], dtype=np.int64)
    n_pos = len(node_start) - 1
    n = int(node_start[-1])
    key = np.asarray(graph["node_key"], dtype=np.uint32).reshape(-1, 6)
    cnt = np.asarray(graph["node_cnt"], dtype=np.int64).reshape(-1, 6)
    assert key.shape[0] == n and cnt.shape[0] == n
    pos = np.repeat(np.arange(n_pos, dtype=np.int64), np.diff(node_start))
    var = np.arange(n, dtype=np.int64) - node_start[pos]
    alive = (key[:, 0] != NONE) | (cnt[:, 0] >= coverage)

    es = np.asarray(graph["edge_start"], dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(es))
    dst = np.asarray(graph["edge_dst"], dtype=np.int64)
    keep = alive[src] & alive[dst]
    pair = np.unique(src[keep] * max(n, 1) + dst[keep])
    src, dst = pair // max(n, 1), pair % max(n, 1)
    assert np.all(pos[dst] > pos[src]), "an alive edge that does not lead to a later position"

    outdeg = np.bincount(src, minlength=n)
    indeg = np.bincount(dst, minlength=n)
    internal = (outdeg[src] == 1) & (indeg[dst] == 1) & (src != dst)

    # rank along the internal edges by pointer jumping
    anc = np.arange(n, dtype=np.int64)
    anc[dst[internal]] = src[internal]
    dist = np.zeros(n, dtype=np.int64)
    dist[dst[internal]] = 1
    for _ in range(64):
        if np.array_equal(anc[anc], anc):
            break
        dist = dist + dist[anc]
        anc = anc[anc]
    assert np.array_equal(anc[anc], anc)
    haspred = np.zeros(n, dtype=bool)
    haspred[dst[internal]] = True
    heads = np.nonzero(alive & ~haspred)[0]
    seg_of_head = np.full(n, -1, dtype=np.int64)
    seg_of_head[heads] = np.arange(len(heads))
    nodes = np.nonzero(alive)[0]
    seg = seg_of_head[anc[nodes]]
    assert np.all(seg >= 0)
    order = np.lexsort((dist[nodes], seg))
    nodes, seg = nodes[order], seg[order]

    if len(nodes):
        assert int(pos[nodes].max()) < len(ref), "an alive node beyond the unit's reference bases"
    votes = cnt[nodes, 1:6]
    best = np.argmax(votes, axis=1)                      # first maximum: A > C > G > T > N
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[best]
    refb = np.frombuffer(bytes(ref), dtype=np.uint8)
    none = votes.sum(axis=1) == 0
    letters = np.where(none, refb[pos[nodes]] if len(nodes) else letters, letters).astype(np.uint8)

    n_seg = len(heads)
    length = np.bincount(seg, minlength=n_seg).astype(np.int64)
    seq_off = np.zeros(n_seg + 1, dtype=np.int64)
    seq_off[1:] = np.cumsum(length)
    cov = np.add.reduceat(cnt[nodes, 0], seq_off[:-1]) if n_seg else np.zeros(0, np.int64)
    last = pos[nodes[seq_off[1:] - 1]] if n_seg else np.zeros(0, np.int64)

    ext = ~internal
    lf, lt = seg_of_head[anc[src[ext]]], seg_of_head[dst[ext]]
    assert np.all(seg_of_head[dst[ext]] >= 0), "a link that does not enter a segment's head"
    lo = np.lexsort((lt, lf))
    return {"head_pos": pos[heads], "head_var": var[heads], "n_nodes": length, "last_pos": last, "coverage": cov, "seq_off": seq_off,
            "seq": letters.tobytes(), "link_from": lf[lo], "link_to": lt[lo]}


def gfa_text(u, unit):
    """The S and L lines of a unitig table (the model's or the engine's) as agx_unitigs_gfa writes them."""
    name = ["u%d_%d_%d" % (unit, p, v) for p, v in zip(u["head_pos"].tolist(), u["head_var"].tolist())]
    off = u["seq_off"].tolist()
    seq = u["seq"]
    out = []
    for s, (nm, ln, kc, pe) in enumerate(zip(name, u["n_nodes"].tolist(), u["coverage"].tolist(), u["last_pos"].tolist())):
        out.append(b"S\t%s\t%s\tLN:i:%d\tKC:i:%d\tpe:i:%d\n" % (nm.encode(), seq[off[s]:off[s + 1]], ln, kc, pe))
    for a, b in zip(u["link_from"].tolist(), u["link_to"].tolist()):
        out.append(b"L\t%s\t+\t%s\t+\t0M\n" % (name[a].encode(), name[b].encode()))
    return b"".join(out)


def unit_gfa(graph, coverage, ref, unit):
    """Expected text of one unit."""
    return gfa_text(unitigs(graph, coverage, ref), unit)


def graph_from_lists(n_per_pos, nodes, edges):
    """A hand-made canonical graph: n_per_pos[x] nodes at position x; nodes[i] = (contig_id or None, coverage, (A, C, G, T, N)) in canonical order;
    edges = (i, j) pairs of canonical indexes (any order, duplicates allowed)."""
    node_start = np.zeros(len(n_per_pos) + 1, dtype=np.uint32)
    node_start[1:] = np.cumsum(n_per_pos)
    n = int(node_start[-1])
    assert len(nodes) == n
    key = np.full((n, 6), NONE, dtype=np.uint32)
    cnt = np.zeros((n, 6), dtype=np.int32)
    for i, (cid, cov, votes) in enumerate(nodes):
        if cid is not None:
            key[i, 0] = cid
        cnt[i, 0] = cov
        cnt[i, 1:6] = votes
    edges = sorted(edges)
    es = np.zeros(n + 1, dtype=np.uint32)
    for a, _ in edges:
        es[a + 1] += 1
    es = np.cumsum(es).astype(np.uint32)
    return {"n_pos": len(n_per_pos), "n_nodes": n, "n_edges": len(edges), "node_start": node_start, "node_key": key, "node_cnt": cnt,
            "node_slen": np.zeros(n, np.uint32), "edge_start": es, "edge_dst": np.array([b for _, b in edges], dtype=np.uint32)}
