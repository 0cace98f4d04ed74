"""numpy model of the paths of an export (DESIGN.md §11 "Paths"): which walk ids have their node in an export and where (the id map of
agx_unit_unitigs_mapped), the pieces of a record's node sequence that stay on edges and inside the map, and the P lines agx_unitigs_paths_gfa writes.

It shares nothing with the kernels or the formatter:

  walk id -> (position, variant)       walk_model.build gives every id's position; the ids of a position are its alive variants in variant order, the main id first
  (position, variant) -> (segment, rank)   unitig_region_model gives the segments by their heads and lengths; a segment's nodes are its head and, one after the
                                       other, the single successor that is alive in the export
  run       maximal stretch of consecutive ids, all main or all side, whose nodes are consecutive nodes of one segment
  path      maximal piece of a record's node sequence (its stretches one after the other) in which every consecutive pair lies inside a stretch or across a
            `joined` boundary and has both nodes in the map
  P line    P <tab> p<unit>_<record>_<first base> <tab> <seg>+,<seg>+,... <tab> * <tab> ln:i:<nodes> <tab> fs:i:<first rank> <tab> ls:i:<last rank>

The stretches themselves (Unit.walk_paths(), or hand-made ones of the same form) are an input: what the walk does is the oracle's business.
"""
import numpy as np

import unitig_model as M
import unitig_region_model as R
import walk_model as WM

NONE = 0xFFFFFFFF


def id_nodes(g, coverage, w=None):
    """Canonical node index of every walk id of a unit built at `coverage` (-1: an id without a node); w: walk_model.build(g, coverage) if the caller has it."""
    w = WM.build(g, coverage) if w is None else w
    n_pos, n_ids = w["n_pos"], w["n_ids"]
    ns = np.asarray(g["node_start"], dtype=np.int64)
    key = np.asarray(g["node_key"], dtype=np.int64).reshape(-1, 6)
    cnt = np.asarray(g["node_cnt"], dtype=np.int64).reshape(-1, 6)
    alive = (key[:, 0] != NONE) | (cnt[:, 0] >= coverage) if len(key) else np.zeros(0, bool)
    alive_idx = np.nonzero(alive)[0]
    before = np.concatenate(([0], np.cumsum(alive)))          # alive nodes in front of node v
    xpos = w["xpos"].astype(np.int64)
    nth = np.zeros(n_ids, np.int64)                            # the id's place among the ids of its position
    sx = xpos[n_pos:]
    assert np.all(np.diff(sx) >= 0), "the side block is not position-major"
    nth[n_pos:] = 1 + np.arange(n_ids - n_pos) - np.searchsorted(sx, sx, side="left")
    node = np.full(n_ids, -1, np.int64)
    has = np.asarray(w["has"], dtype=bool)
    node[has] = alive_idx[before[ns[xpos[has]]] + nth[has]]
    pos_of = np.repeat(np.arange(len(ns) - 1, dtype=np.int64), np.diff(ns))
    assert np.array_equal(pos_of[node[has]], xpos[has])
    return node


def node_places(g, lo, hi, min_cov, ref):
    """The export of window [lo, hi) at min_cov (unitig_region_model) and, per canonical node, its segment and rank there (-1: not in the export)."""
    rg = R.region_graph(g, lo, hi)
    u = M.unitigs(rg, min_cov, ref)
    ns = np.asarray(rg["node_start"], dtype=np.int64)
    n = int(ns[-1])
    key, cnt = rg["node_key"], rg["node_cnt"]
    alive = (key[:, 0] != NONE) | (cnt[:, 0] >= min_cov) if n else np.zeros(0, bool)
    es = np.asarray(rg["edge_start"], dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(es))
    dst = np.asarray(rg["edge_dst"], dtype=np.int64)
    keep = alive[src] & alive[dst] if len(src) else np.zeros(0, bool)
    pair = np.unique(src[keep] * max(n, 1) + dst[keep])
    src, dst = pair // max(n, 1), pair % max(n, 1)
    only = np.full(n, -1, np.int64)
    only[src] = dst                                            # (read only where a segment goes on: the node then has one alive successor)
    outdeg = np.bincount(src, minlength=n)
    seg, rank = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    cur = ns[u["head_pos"].astype(np.int64)] + u["head_var"].astype(np.int64)
    sidx = np.arange(len(cur), dtype=np.int64)
    length = np.asarray(u["n_nodes"], dtype=np.int64)
    r = 0
    while len(cur):
        assert np.all(seg[cur] < 0), "two segments share a node"
        seg[cur], rank[cur] = sidx, r
        go = r + 1 < length[sidx]
        assert np.all(outdeg[cur[go]] == 1)
        cur, sidx = only[cur[go]], sidx[go]
        r += 1
    assert np.array_equal(seg >= 0, alive)
    return u, seg, rank


def entries(g, coverage, lo, hi, min_cov, ref, w=None):
    """(export, segment per walk id, rank per walk id); -1 where the id has no node in the export."""
    node = id_nodes(g, coverage, w)
    u, seg, rank = node_places(g, lo, hi, min_cov, ref)
    on = node >= 0
    e_seg, e_rank = np.full(len(node), -1, np.int64), np.full(len(node), -1, np.int64)
    e_seg[on], e_rank[on] = seg[node[on]], rank[node[on]]
    return u, e_seg, e_rank


def runs_of(e_seg, e_rank, n_pos):
    """The id map as the engine hands it out: id_first, id_last, seg, rank_first per run."""
    n = len(e_seg)
    present = e_seg >= 0
    cont = np.zeros(n, bool)                                   # id i continues id i - 1
    if n > 1:
        cont[1:] = present[1:] & present[:-1] & (e_seg[1:] == e_seg[:-1]) & (e_rank[1:] == e_rank[:-1] + 1)
    if n_pos < n:
        cont[n_pos] = False                                    # a run never holds a main id and a side id
    first = np.nonzero(present & ~cont)[0]
    last = np.nonzero(present & ~np.concatenate((cont[1:], [False])))[0]
    assert len(first) == len(last)
    return {"n_pos": n_pos, "n_ids": n, "id_first": first.astype(np.uint32), "id_last": last.astype(np.uint32),
            "seg": e_seg[first].astype(np.uint32), "rank_first": e_rank[first].astype(np.uint32)}


def id_map(g, coverage, lo, hi, min_cov, ref, w=None):
    """The model's side of Unit.unitigs(region=(lo, hi), min_coverage=min_cov, id_map=True): the export with its "id_map" entry."""
    u, e_seg, e_rank = entries(g, coverage, lo, hi, min_cov, ref, w)
    u = dict(u)
    u["id_map"] = runs_of(e_seg, e_rank, int(g["n_pos"]))
    return u, e_seg, e_rank


def paths(u, e_seg, e_rank, w):
    """The paths of the records of w (the dict Unit.walk_paths() returns) over the export u, node by node: dicts rec, base, segs, ln, fs, ls in (record, first base) order."""
    links = set(zip(np.asarray(u["link_from"]).tolist(), np.asarray(u["link_to"]).tolist()))
    length = np.asarray(u["n_nodes"]).tolist()
    es, er = np.asarray(e_seg).tolist(), np.asarray(e_rank).tolist()
    st_off = np.asarray(w["st_off"]).tolist()
    first, last, base, joined = (np.asarray(w[k]).tolist() for k in ("id_first", "id_last", "base_off", "joined"))
    out = []
    for r in range(len(w["rec_len"])):
        prev = None                                            # (segment, rank) of the node in front, if this one follows it over an edge and it is in the map
        for i in range(st_off[r], st_off[r + 1]):
            if not joined[i]:
                prev = None
            for a in range(first[i], last[i] + 1):
                s, k = es[a], er[a]
                if s < 0:
                    prev = None
                    continue
                if prev is None:
                    out.append({"rec": r, "base": base[i] + (a - first[i]), "segs": [s], "ln": 1, "fs": k, "ls": k})
                else:
                    ps, pk = prev
                    if not (s == ps and k == pk + 1):
                        assert pk + 1 == length[ps] and k == 0 and (ps, s) in links, "record %d: id %d does not follow its predecessor in the export" % (r, a)
                        out[-1]["segs"].append(s)
                    out[-1]["ln"] += 1
                    out[-1]["ls"] = k
                prev = (s, k)
    return out


def p_text(u, ps, unit):
    name = ["u%d_%d_%d" % (unit, p, v) for p, v in zip(np.asarray(u["head_pos"]).tolist(), np.asarray(u["head_var"]).tolist())]
    return b"".join(b"P\tp%d_%d_%d\t%s\t*\tln:i:%d\tfs:i:%d\tls:i:%d\n" % (unit, p["rec"], p["base"], ",".join(name[s] + "+" for s in p["segs"]).encode(), p["ln"], p["fs"], p["ls"])
                    for p in ps)


def paths_gfa(u, e_seg, e_rank, w, unit):
    """Expected P lines of one unit."""
    return p_text(u, paths(u, e_seg, e_rank, w), unit)


def stretches(recs):
    """Hand-made stretches in the form of Unit.walk_paths(): recs = [(record length, [(id_first, id_last, base_off, joined), ...]), ...]."""
    st_off, rows = [0], []
    for _, st in recs:
        rows += st
        st_off.append(len(rows))
    col = lambda j, dt: np.array([x[j] for x in rows], dtype=dt)
    return {"rec_len": np.array([n for n, _ in recs], np.uint64), "st_off": np.array(st_off, np.uint64), "id_first": col(0, np.uint32), "id_last": col(1, np.uint32),
            "base_off": col(2, np.uint64), "joined": col(3, np.uint8)}


def fasta_records(text):
    """The sequences of a FASTA text (pre_extended), in order."""
    return [b"".join(rec.split(b"\n")[1:]) for rec in text.split(b">")[1:]]
