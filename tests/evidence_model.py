"""numpy model of the evidence under the walk's records (agx_unit_walk_evidence), over the oracle's graph dump.

It shares nothing with the lane function or the kernels:

  walk id -> node          path_model.id_nodes (the walk model's numbering of the alive nodes)
  depth, votes             the oracle's node_cnt: column 0, and the largest of columns 1 .. 5
  step                     edge_support_model.support's count of the edge between the two nodes (edge_support_of); None there = the graph has no such edge
  records, intervals       a loop over every base

The stretches (Unit.walk_paths(), or hand-made ones from path_model.stretches) are an input.  `sup` is what edge_support_model.support returns, or any dict with
edge_start / edge_dst / edge_cnt in agx_unit_graph's numbering; None models a unit without edge counters: every step is NONE.
"""
import numpy as np

import edge_support_model as ESM
import path_model as PM

NONE = 0xFFFFFFFF
REC_KEYS = ("rec_graph_bases", "rec_steps", "rec_depth_sum", "rec_depth_min", "rec_depth_min_at", "rec_step_min", "rec_step_min_at")
IV_KEYS = ("iv_rec", "iv_first", "iv_last", "iv_depth_min", "iv_step_min")
TOTALS = ("n_graph_bases", "n_steps", "n_steps_without_edge")
TRACK_KEYS = ("track_off", "depth", "votes", "step")


def bases(g, coverage, w, sup=None, wm=None, node=None):
    """Every graph base in (record, stretch, base) order: lists rec, off, depth, votes, step; the first entry of every stretch; the steps without an edge."""
    node = PM.id_nodes(g, coverage, wm) if node is None else node
    cnt = np.asarray(g["node_cnt"], dtype=np.int64).reshape(-1, 6)
    st_off = np.asarray(w["st_off"]).astype(np.int64).tolist()
    first, last, base, joined = (np.asarray(w[k]).astype(np.int64).tolist() for k in ("id_first", "id_last", "base_off", "joined"))
    rec, off, depth, votes, step, track_off = [], [], [], [], [], []
    no_edge = 0
    for r in range(len(w["rec_len"])):
        for i in range(st_off[r], st_off[r + 1]):
            track_off.append(len(rec))
            for a in range(first[i], last[i] + 1):
                v = int(node[a]) if a < len(node) else -1
                if a < last[i]:
                    t = a + 1
                elif i + 1 < st_off[r + 1] and joined[i + 1]:
                    t = first[i + 1]
                else:
                    t = None
                s = NONE
                if t is not None and sup is not None and v >= 0 and t < len(node) and node[t] >= 0:
                    c = ESM.edge_support_of(sup, v, int(node[t]))
                    if c is None:
                        no_edge += 1
                    else:
                        s = c
                rec.append(r)
                off.append(base[i] + (a - first[i]))
                depth.append(NONE if v < 0 else int(cnt[v, 0]))
                votes.append(NONE if v < 0 else int(cnt[v, 1:].max()))
                step.append(s)
    track_off.append(len(rec))
    return rec, off, depth, votes, step, track_off, no_edge


def evidence(g, coverage, w, sup=None, min_depth=0, min_support=0, records=None, wm=None, node=None):
    """The model's side of Unit.walk_evidence(w, min_depth, min_support, tracks=True, records=records): the same dict."""
    rec, off, depth, votes, step, track_off, no_edge = bases(g, coverage, w, sup, wm, node)
    nr = len(w["rec_len"])
    out = {"n_graph_bases": len(rec), "n_steps": sum(1 for s in step if s != NONE), "n_steps_without_edge": no_edge}
    R = {k: [0] * nr for k in REC_KEYS}
    for r in range(nr):
        R["rec_depth_min"][r] = R["rec_step_min"][r] = NONE
    for r, o, d, s in zip(rec, off, depth, step):
        R["rec_graph_bases"][r] += 1
        if d != NONE:
            R["rec_depth_sum"][r] += d
            if d < R["rec_depth_min"][r]:
                R["rec_depth_min"][r], R["rec_depth_min_at"][r] = d, o
        if s != NONE:
            R["rec_steps"][r] += 1
            if s < R["rec_step_min"][r]:
                R["rec_step_min"][r], R["rec_step_min_at"][r] = s, o
    for k in REC_KEYS:
        out[k] = np.array(R[k], np.uint64 if k in REC_KEYS[:3] else np.uint32)
    iv = []
    for r, o, d, s in zip(rec, off, depth, step):
        if not (d == NONE or d < min_depth or (s != NONE and s < min_support)):
            continue
        if iv and iv[-1][0] == r and iv[-1][2] + 1 == o:
            iv[-1][2] = o
            iv[-1][3] = min(iv[-1][3], d)
            iv[-1][4] = min(iv[-1][4], s)
        else:
            iv.append([r, o, o, d, s])
    for j, k in enumerate(IV_KEYS):
        out[k] = np.array([x[j] for x in iv], np.uint32)
    lo, hi = (0, nr) if records is None else records
    st_off = np.asarray(w["st_off"]).astype(np.int64)
    s_lo, s_hi = (int(st_off[lo]), int(st_off[hi])) if len(st_off) else (0, 0)
    a, b = track_off[s_lo], track_off[s_hi]
    out.update(rec_lo=lo, rec_hi=hi, track_off=np.array(track_off[s_lo:s_hi + 1], np.uint64) - np.uint64(a),
               depth=np.array(depth[a:b], np.uint32), votes=np.array(votes[a:b], np.uint32), step=np.array(step[a:b], np.uint32))
    return out


def same(got, want, tracks=False):
    """Field by field; returns the first field that differs, or None."""
    for k in TOTALS:
        if int(got[k]) != int(want[k]):
            return k
    for k in REC_KEYS + IV_KEYS + (TRACK_KEYS if tracks else ()):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            return k
    return None


def bed(e, unit):
    """Expected BED text of the weak intervals of e."""
    num = lambda v: b"." if int(v) == NONE else b"%d" % int(v)
    return b"".join(b"p%d_%d\t%d\t%d\tweak\t0\t+\tdm:i:%s\tsm:i:%s\n" % (unit, r, a, b + 1, num(d), num(s))
                    for r, a, b, d, s in zip(*(np.asarray(e[k]).tolist() for k in IV_KEYS)))
