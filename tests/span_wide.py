"""A second, wide reference of the pair span for units of hundreds of thousands of hits, where the loops of tests/span_model.py are too slow.

Plain numpy; nothing of the project is imported, tests/span_model.py included.  It does not do what the kernels do (scatter to start / end and scan) and not what the
model does (a loop over the hits, a slice increment per fragment, a count over all fragments per base):

  fragments    every field of dhit as one array; a simple mate covers [t0, t0 + len - 1]; the mates with runs take the smallest t and the largest t + n - 1 of their runs by
               one reduction over a flat copy of their pieces of the run table
  span, cross  counted from the sorted endpoints: span[x] = #(f_lo <= x) - #(f_hi < x), cross[x] = #(f_lo <= x) - #(f_hi <= x), by np.searchsorted
  bases        the stretch table flattened into arrays; a step to the neighbouring position is cross[x], a jump one count over the fragments per distinct (x, y)

fragments_at() also says which record each fragment came from, for the tests that must know what the records behind a given index hold.  Input and output are the model's:
the front of a unit (dhit, runs, n_pos) in any order, and the same tuples and dicts, so that span_model.walk_span(..., based=bases(...)) makes the expected answer.
"""
import numpy as np

NONE = 0xFFFFFFFF
HF_SKIP = 2
BIG = np.int64(1) << 62


def _mate(t0, first_run, n_mate_runs, length, runs):
    """(lo, hi) of one mate of every hit: its smallest and largest aligned position (int64; BIG and -1 for a mate that covers nothing)."""
    simple = (n_mate_runs == 0) & (length > 0)
    lo, hi = np.where(simple, t0, BIG), np.where(simple, t0 + length - 1, -1)
    cnt = np.minimum(n_mate_runs, np.maximum(len(runs) - first_run, 0))      # (a run index at or behind the table's end names no run)
    who = np.nonzero(cnt > 0)[0]
    if len(who):
        cnt, first = cnt[who], first_run[who]
        seg = np.concatenate(([0], np.cumsum(cnt)[:-1]))
        at = np.repeat(first - seg, cnt) + np.arange(int(cnt.sum()))        # the run indexes of every such mate, one mate after the other
        t, n = runs["t"].astype(np.int64)[at], runs["n"].astype(np.int64)[at]
        lo[who] = np.minimum.reduceat(np.where(n > 0, t, BIG), seg)         # (a run of no bases covers nothing)
        hi[who] = np.maximum.reduceat(np.where(n > 0, t + n - 1, -1), seg)
    return lo, hi


def mates(front):
    """Per hit record: a_lo, a_hi, b_lo, b_hi (the aligned bounds of each mate, not clamped), kept (bool), with_runs (bool: a mate of the hit has runs)."""
    d, runs = front["dhit"], front["runs"]
    f = {k: d[k].astype(np.int64) for k in ("a_t0", "b_t0", "a_runs", "b_runs", "len", "a_nruns", "b_nruns", "flags")}
    a_lo, a_hi = _mate(f["a_t0"], f["a_runs"], f["a_nruns"], f["len"], runs)
    b_lo, b_hi = _mate(f["b_t0"], f["b_runs"], f["b_nruns"], f["len"], runs)
    return a_lo, a_hi, b_lo, b_hi, (f["flags"] & HF_SKIP) == 0, (f["a_nruns"] > 0) | (f["b_nruns"] > 0)


def fragments_at(front):
    """(f_lo, f_hi, record index of each fragment, kept: a bool per record, outside: a bool per record), fragments in the order of the records."""
    n_pos = int(front["n_pos"])
    a_lo, a_hi, b_lo, b_hi, kept, _ = mates(front)
    lo, hi = np.minimum(a_lo, b_lo), np.maximum(a_hi, b_hi)
    outside = kept & (lo >= n_pos)
    has = kept & ~outside
    return lo[has], np.minimum(hi[has], n_pos - 1), np.nonzero(has)[0], kept, outside


def fragments(front):
    """(f_lo, f_hi as int64 arrays over the kept hits that have a fragment, n_kept, n_outside): span_model.fragments' four values"""
    f_lo, f_hi, _, kept, outside = fragments_at(front)
    return f_lo, f_hi, int(kept.sum()), int(outside.sum())


def unit_span(front, frags=None):
    """span and cross of every position (int64), from the sorted endpoints."""
    f_lo, f_hi = (frags if frags is not None else fragments(front))[:2]
    x = np.arange(int(front["n_pos"]), dtype=np.int64)
    lo_s, hi_s = np.sort(f_lo), np.sort(f_hi)
    begun = np.searchsorted(lo_s, x, side="right").astype(np.int64)         # #(f_lo <= x)
    return begun - np.searchsorted(hi_s, x, side="left"), begun - np.searchsorted(hi_s, x, side="right")


def pairs(frags, x, y):
    """The fragments with f_lo <= x and y <= f_hi (x < y)."""
    assert x < y
    return int(np.count_nonzero((frags[0] <= x) & (frags[1] >= y)))


def pair_span(front, region=None, frags=None, spans=None):
    """The reference's side of Unit.pair_span(region): the same dict as span_model.pair_span.  spans: what unit_span() returned for these fragments, to spare the sorts."""
    frags = fragments(front) if frags is None else frags
    n_pos = int(front["n_pos"])
    lo, hi = (0, n_pos) if region is None else region
    span, cross = unit_span(front, frags) if spans is None else spans
    meets = int(np.count_nonzero((frags[0] < hi) & (frags[1] >= lo))) if lo < hi else 0
    return {"pos_lo": lo, "pos_hi": hi, "n_kept": frags[2], "n_fragments": meets, "n_outside": frags[3], "span": span[lo:hi].astype(np.uint32), "cross": cross[lo:hi].astype(np.uint32)}


def bases(front, side_xpos, w, frags=None):
    """Every graph base in (record, stretch, base) order: lists rec, off, pos, span, step; the first entry of every stretch; jump steps; steps not forward —
    span_model.bases' tuple."""
    frags = fragments(front) if frags is None else frags
    n_pos = int(front["n_pos"])
    span_all, cross_all = unit_span(front, frags)
    st_off = np.asarray(w["st_off"]).astype(np.int64)
    first, last, base, joined = (np.asarray(w[k]).astype(np.int64) for k in ("id_first", "id_last", "base_off", "joined"))
    nr = len(w["rec_len"])
    n_of = st_off[1:nr + 1] - st_off[:nr]                                    # stretches of each record
    r_seg = np.concatenate(([0], np.cumsum(n_of)))
    st = np.repeat(st_off[:nr] - r_seg[:-1], n_of) + np.arange(int(r_seg[-1]))      # the stretches in (record, stretch) order
    st_rec = np.repeat(np.arange(nr), n_of)
    n_b = last[st] - first[st] + 1
    track_off = np.concatenate(([0], np.cumsum(n_b)))
    k = np.arange(int(track_off[-1])) - np.repeat(track_off[:-1], n_b)       # offset of each base inside its stretch
    s_of = np.repeat(st, n_b)
    a = first[s_of] + k
    # the step's target: the next id of the stretch, else the first id of a joined next stretch of the same record, else none
    nxt = s_of + 1
    joins = (nxt < np.repeat(np.repeat(st_off[1:nr + 1], n_of), n_b)) & (joined[np.minimum(nxt, max(len(joined) - 1, 0))] != 0 if len(joined) else False)
    inner = a < last[s_of]
    t = np.where(inner, a + 1, np.where(joins, first[np.minimum(nxt, max(len(first) - 1, 0))] if len(first) else 0, -1))
    side = np.asarray(side_xpos).astype(np.int64)

    def position(ids):
        out = ids.copy()
        far = ids >= n_pos
        out[far] = side[ids[far] - n_pos]
        return out
    x = position(a)
    has = t >= 0
    y = np.full(len(a), -1, np.int64)
    y[has] = position(t[has])
    fwd = has & (y > x)
    step = np.full(len(a), NONE, np.int64)
    nb = fwd & (y == x + 1)
    step[nb] = cross_all[x[nb]]
    jump = fwd & (y > x + 1)
    if jump.any():
        xy, inv = np.unique(np.stack((x[jump], y[jump]), 1), axis=0, return_inverse=True)
        cnt = np.array([pairs(frags, int(p), int(q)) for p, q in xy], np.int64)
        step[jump] = cnt[np.asarray(inv).reshape(-1)]
    return (np.repeat(st_rec, n_b).tolist(), (base[s_of] + k).tolist(), x.tolist(), span_all[x].tolist(), step.tolist(), track_off.tolist(),
            int(jump.sum()), int((has & ~fwd).sum()))
