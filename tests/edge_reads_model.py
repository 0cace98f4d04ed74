"""Edge reads, the reference's way: WHICH hits name each edge of a unit's graph.

Plain Python / numpy; of the project only tests/edge_support_model.py is imported, and it is followed step by step: the update_kmer calls of every kept hit
(events_of_hit over the mates' position_sets), the variants the candidate keys of both ends resolve to (_variants), every pair of them that passes the
contig-consistency test — but where support() counts the events of a pair, reads() keeps the number of the hit each event belongs to.  A hit's number is its index in the
front's dhit in file order.

reads(front, graph, k, iv) -> {(src, dst): sorted list of hit numbers}, src / dst in the oracle's canonical node ids (agx_unit_graph's numbering).
pos_var(graph, ids) -> (position, variant index at the position) of canonical ids.
table(reads, graph, lo, hi, max_support) -> the selection of a window as agx_unit_edge_reads lays it out: the edges whose source position lies in [lo, hi) and whose
support is <= max_support, by (src_pos, src_var, dst_pos, dst_var), with support, hit_off and hit.
"""
import numpy as np

import edge_support_model as ESM

NONE = ESM.NONE
ALL = 0xFFFFFFFF
EDGE_KEYS = ("src_pos", "src_var", "dst_pos", "dst_var", "support")


def events_with_hits(front, k):
    """ESM.events with the owner of every row: ([n, 4] events, [n] hit numbers)."""
    runs, rows, owner = front["runs"], [], []
    for h, d in enumerate(front["dhit"]):
        if int(d["flags"]) & ESM.HF_SKIP:
            continue
        L = int(d["len"])
        pa = ESM.position_set(int(d["a_t0"]), int(d["a_runs"]), int(d["a_nruns"]), runs, L)
        pb = ESM.position_set(int(d["b_t0"]), int(d["b_runs"]), int(d["b_nruns"]), runs, L)
        ev = ESM.events_of_hit(pa, pb, k)
        rows.append(ev)
        owner.append(np.full(len(ev), h, np.int64))
    if not rows:
        return np.zeros((0, 4), np.int64), np.zeros(0, np.int64)
    return np.concatenate(rows), np.concatenate(owner)


def reads(front, graph, k, iv):
    E, H = events_with_hits(front, k)
    if not len(E):
        return {}
    ev_s, id_s = ESM._variants(E[:, 0], E[:, 2], graph, front["cm_start"], front["cm"], iv)
    ev_d, id_d = ESM._variants(E[:, 1], E[:, 3], graph, front["cm_start"], front["cm"], iv)
    cd = np.bincount(ev_d, minlength=len(E))                 # S x D per event, as support() lays it out
    start_d = np.cumsum(cd) - cd
    rep = cd[ev_s]
    s_rows = np.repeat(np.arange(len(ev_s)), rep)
    kth = np.arange(len(s_rows)) - np.repeat(np.cumsum(rep) - rep, rep)
    src, dst, ev = id_s[s_rows], id_d[start_d[ev_s[s_rows]] + kth], ev_s[s_rows]
    key = graph["node_key"].astype(np.int64)
    a, b = key[src], key[dst]
    allowed = ESM._clause_ab(b[:, 0], b[:, 1], a[:, 0], a[:, 1], ESM.EP25) & ESM._clause_ab(b[:, 2], b[:, 3], a[:, 2], a[:, 3], 2 * iv + ESM.EP25)
    out = {}
    for s, d, h in zip(src[allowed].tolist(), dst[allowed].tolist(), H[ev[allowed]].tolist()):
        out.setdefault((s, d), []).append(h)
    return {e: sorted(hs) for e, hs in out.items()}


def pos_var(graph, ids):
    ns = graph["node_start"].astype(np.int64)
    ids = np.asarray(ids, np.int64)
    pos = np.searchsorted(ns, ids, side="right") - 1
    return pos, ids - ns[pos]


def table(rd, graph, lo=0, hi=None, max_support=ALL):
    hi = int(graph["n_pos"]) if hi is None else hi
    edges = sorted(rd)
    sp, sv = pos_var(graph, [e[0] for e in edges]) if edges else (np.zeros(0, np.int64),) * 2
    dp, dv = pos_var(graph, [e[1] for e in edges]) if edges else (np.zeros(0, np.int64),) * 2
    rows = sorted((int(sp[i]), int(sv[i]), int(dp[i]), int(dv[i]), edges[i]) for i in range(len(edges))
                  if lo <= sp[i] < hi and len(rd[edges[i]]) <= max_support)
    out = {k: np.array([r[j] for r in rows], np.uint32) for j, k in enumerate(EDGE_KEYS[:4])}
    out["support"] = np.array([len(rd[r[4]]) for r in rows], np.uint32)
    out["hit_off"] = np.concatenate([[0], np.cumsum(out["support"], dtype=np.uint64)]).astype(np.uint64)
    out["hit"] = np.array([h for r in rows for h in rd[r[4]]], np.uint32)
    return out


def same(got, want):
    """None, or the first field in which two tables differ."""
    for k in EDGE_KEYS + ("hit_off", "hit"):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            return k
    return None
