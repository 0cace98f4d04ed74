"""numpy model of the pair span (agx_unit_pair_span, agx_unit_walk_span).

Plain Python / numpy; nothing of the project is imported.  Input: the front of a unit in file order (hostsim sim.run(..., front=True)["front"]: dhit, runs, n_pos) —
the order does not matter, every number here is a count over all kept hits.

  fragment of a kept hit   a loop over the hits: the aligned positions of both mates (a simple mate: t0 .. t0 + len - 1; else the union of its runs; a_runs is ignored
                           where both run counts are 0), their minimum and maximum, the maximum clamped to n_pos - 1; a hit that begins at or behind n_pos is "outside"
  span, cross              a loop over the fragments, one slice increment each
  pairs(x, y)              a direct count over all fragments
  the walk join            a loop over every base of the stretch table; positions from side_xpos (the walk model's: walk_model.build(...)["side_xpos"]), an input
"""
import numpy as np

NONE = 0xFFFFFFFF
HF_SKIP = 2
REC_KEYS = ("rec_graph_bases", "rec_steps", "rec_span_sum", "rec_span_min", "rec_span_min_at", "rec_step_min", "rec_step_min_at")
IV_KEYS = ("iv_rec", "iv_first", "iv_last", "iv_span_min", "iv_step_min")
TOTALS = ("n_graph_bases", "n_steps", "n_jump_steps", "n_steps_not_forward")
TRACK_KEYS = ("track_off", "pos", "span", "step")
SPAN_KEYS = ("pos_lo", "pos_hi", "n_kept", "n_fragments", "n_outside")


def mate_positions(t0, first_run, n_runs, runs, L):
    """(smallest, largest) aligned position of one mate, or None if it covers nothing."""
    if n_runs == 0:
        return (t0, t0 + L - 1) if L else None
    lo = hi = None
    for r in runs[first_run:first_run + n_runs]:
        t, n = int(r["t"]), int(r["n"])
        if n:
            lo = t if lo is None else min(lo, t)
            hi = t + n - 1 if hi is None else max(hi, t + n - 1)
    return None if lo is None else (lo, hi)


def fragments(front):
    """(f_lo, f_hi as int64 arrays over the kept hits that have a fragment, n_kept, n_outside)"""
    n_pos, runs = int(front["n_pos"]), front["runs"]
    lo, hi, kept, outside = [], [], 0, 0
    for d in front["dhit"]:
        if int(d["flags"]) & HF_SKIP:
            continue
        kept += 1
        L = int(d["len"])
        simple = int(d["a_nruns"]) == 0 and int(d["b_nruns"]) == 0
        m = [mate_positions(int(d["a_t0"]), 0 if simple else int(d["a_runs"]), int(d["a_nruns"]), runs, L),
             mate_positions(int(d["b_t0"]), 0 if simple else int(d["b_runs"]), int(d["b_nruns"]), runs, L)]
        m = [x for x in m if x is not None]
        f_lo = min(x[0] for x in m) if m else n_pos
        if f_lo >= n_pos:
            outside += 1
            continue
        lo.append(f_lo)
        hi.append(min(max(x[1] for x in m), n_pos - 1))
    return np.array(lo, np.int64), np.array(hi, np.int64), kept, outside


def pairs(frags, x, y):
    """The fragments with f_lo <= x and y <= f_hi (x < y)."""
    assert x < y
    return int(((frags[0] <= x) & (y <= frags[1])).sum())


def unit_span(front, frags=None):
    """span and cross of every position (int64)."""
    f_lo, f_hi = (frags if frags is not None else fragments(front))[:2]
    n_pos = int(front["n_pos"])
    span, ends = np.zeros(n_pos, np.int64), np.zeros(n_pos, np.int64)
    for a, b in zip(f_lo.tolist(), f_hi.tolist()):
        span[a:b + 1] += 1
        ends[b] += 1
    return span, span - ends


def pair_span(front, region=None, frags=None):
    """The model's side of Unit.pair_span(region): the same dict."""
    frags = fragments(front) if frags is None else frags
    n_pos = int(front["n_pos"])
    lo, hi = (0, n_pos) if region is None else region
    span, cross = unit_span(front, frags)
    meets = int(((frags[0] < hi) & (frags[1] >= lo)).sum()) if lo < hi else 0
    return {"pos_lo": lo, "pos_hi": hi, "n_kept": frags[2], "n_fragments": meets, "n_outside": frags[3], "span": span[lo:hi].astype(np.uint32), "cross": cross[lo:hi].astype(np.uint32)}


def same_span(got, want):
    """Field by field; returns the first field that differs, or None."""
    for k in SPAN_KEYS:
        if int(got[k]) != int(want[k]):
            return k
    for k in ("span", "cross"):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            return k
    return None


def position(a, n_pos, side_xpos):
    return a if a < n_pos else int(side_xpos[a - n_pos])


def bases(front, side_xpos, w, frags=None):
    """Every graph base in (record, stretch, base) order: lists rec, off, pos, span, step; the first entry of every stretch; jump steps; steps not forward."""
    frags = fragments(front) if frags is None else frags
    n_pos = int(front["n_pos"])
    span_all, cross_all = unit_span(front, frags)
    st_off = np.asarray(w["st_off"]).astype(np.int64).tolist()
    first, last, base, joined = (np.asarray(w[k]).astype(np.int64).tolist() for k in ("id_first", "id_last", "base_off", "joined"))
    rec, off, pos, span, step, track_off = [], [], [], [], [], []
    jumps = back = 0
    for r in range(len(w["rec_len"])):
        for i in range(st_off[r], st_off[r + 1]):
            track_off.append(len(rec))
            for a in range(first[i], last[i] + 1):
                if a < last[i]:
                    t = a + 1
                elif i + 1 < st_off[r + 1] and joined[i + 1]:
                    t = first[i + 1]
                else:
                    t = None
                x = position(a, n_pos, side_xpos)
                s = NONE
                if t is not None:
                    y = position(t, n_pos, side_xpos)
                    if y <= x:
                        back += 1
                    else:
                        s = pairs(frags, x, y)
                        jumps += y > x + 1
                        if y == x + 1:
                            assert s == int(cross_all[x])
                rec.append(r)
                off.append(base[i] + (a - first[i]))
                pos.append(x)
                span.append(int(span_all[x]))
                step.append(s)
    track_off.append(len(rec))
    return rec, off, pos, span, step, track_off, jumps, back


def walk_span(front, side_xpos, w, min_span=0, records=None, frags=None, based=None):
    """The model's side of Unit.walk_span(w, min_span, tracks=True, records=records): the same dict.  based: what bases() returned for this table (it does not depend on
    min_span or records), to spare the loop over the bases."""
    rec, off, pos, span, step, track_off, jumps, back = bases(front, side_xpos, w, frags) if based is None else based
    nr = len(w["rec_len"])
    out = {"n_graph_bases": len(rec), "n_steps": sum(1 for s in step if s != NONE), "n_jump_steps": jumps, "n_steps_not_forward": back}
    R = {k: [0] * nr for k in REC_KEYS}
    for r in range(nr):
        R["rec_span_min"][r] = R["rec_step_min"][r] = NONE
    for r, o, d, s in zip(rec, off, span, step):
        R["rec_graph_bases"][r] += 1
        R["rec_span_sum"][r] += d
        if d < R["rec_span_min"][r]:
            R["rec_span_min"][r], R["rec_span_min_at"][r] = d, o
        if s != NONE:
            R["rec_steps"][r] += 1
            if s < R["rec_step_min"][r]:
                R["rec_step_min"][r], R["rec_step_min_at"][r] = s, o
    for k in REC_KEYS:
        out[k] = np.array(R[k], np.uint64 if k in REC_KEYS[:3] else np.uint32)
    iv = []
    for r, o, d, s in zip(rec, off, span, step):
        if not (d < min_span or (s != NONE and s < min_span)):
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
               pos=np.array(pos[a:b], np.uint32), span=np.array(span[a:b], np.uint32), step=np.array(step[a:b], np.uint32))
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
    """Expected BED text of the thin intervals of e."""
    num = lambda v: b"." if int(v) == NONE else b"%d" % int(v)
    return b"".join(b"p%d_%d\t%d\t%d\tthin\t0\t+\tpm:i:%s\tjm:i:%s\n" % (unit, r, a, b + 1, num(d), num(s))
                    for r, a, b, d, s in zip(*(np.asarray(e[k]).tolist() for k in IV_KEYS)))
