"""numpy model of the mate links (agx_unit_mate_links).

Plain Python / numpy; nothing of the project is imported.  Input: the fragments of a unit as span_model.fragments(front) returns them (f_lo, f_hi, n_kept, n_outside),
the unit's n_pos and side_xpos, and a stretch table.

  own          a loop over every graph base of the table: the smallest record number on its position (a main id is its position, a side id has it in side_xpos)
  the classes  a loop over the fragments: A = own[f_lo], B = own[f_hi]
  the links    a dict (A, B) -> [n_pairs, len_sum, lo_min, lo_max, hi_min, hi_max]
"""
import numpy as np

NONE = 0xFFFFFFFF
TOTALS = ("n_kept", "n_outside", "n_fragments", "n_unowned", "n_inside", "n_open", "n_link_pairs", "n_links_all", "n_owned", "n_shadowed")
REC_KEYS = ("rec_inside", "rec_open_left", "rec_open_right", "rec_links_out", "rec_links_in")
LINK_KEYS = ("a", "b", "n_pairs", "len_sum", "lo_min", "lo_max", "hi_min", "hi_max")


def base_positions(n_pos, side_xpos, w):
    """(record, position) of every graph base, in the table's order"""
    st_off = np.asarray(w["st_off"]).astype(np.int64).tolist()
    first, last = (np.asarray(w[k]).astype(np.int64).tolist() for k in ("id_first", "id_last"))
    out = []
    for r in range(len(w["rec_len"])):
        for i in range(st_off[r], st_off[r + 1]):
            for a in range(first[i], last[i] + 1):
                out.append((r, a if a < n_pos else int(side_xpos[a - n_pos])))
    return out


def owners(n_pos, side_xpos, w):
    """(own as a list over the positions with NONE for nobody, n_owned, n_shadowed)"""
    own = [NONE] * n_pos
    bases = base_positions(n_pos, side_xpos, w)
    for r, x in bases:
        if r < own[x]:
            own[x] = r
    return own, sum(1 for o in own if o != NONE), sum(1 for r, x in bases if own[x] != r)


def mate_links(frags, n_pos, side_xpos, w, min_pairs=1):
    """The model's side of Unit.mate_links(w, min_pairs): the same dict, less n_passes and n_slots."""
    f_lo, f_hi, kept, outside = frags
    nr = len(w["rec_len"])
    own, n_owned, n_shadowed = owners(n_pos, side_xpos, w)
    R = {k: [0] * nr for k in REC_KEYS}
    T = dict.fromkeys(("n_unowned", "n_inside", "n_open", "n_link_pairs"), 0)
    links = {}
    for lo, hi in zip(np.asarray(f_lo).tolist(), np.asarray(f_hi).tolist()):
        a, b = own[lo], own[hi]
        if a == NONE and b == NONE:
            T["n_unowned"] += 1
        elif a == b:
            T["n_inside"] += 1
            R["rec_inside"][a] += 1
        elif b == NONE:
            T["n_open"] += 1
            R["rec_open_right"][a] += 1
        elif a == NONE:
            T["n_open"] += 1
            R["rec_open_left"][b] += 1
        else:
            T["n_link_pairs"] += 1
            R["rec_links_out"][a] += 1
            R["rec_links_in"][b] += 1
            if (a, b) not in links:
                links[(a, b)] = [0, 0, lo, lo, hi, hi]
            v = links[(a, b)]
            v[0] += 1
            v[1] += hi - lo + 1
            v[2], v[3], v[4], v[5] = min(v[2], lo), max(v[3], lo), min(v[4], hi), max(v[5], hi)
    out = dict(T, n_kept=kept, n_outside=outside, n_fragments=len(f_lo), n_links_all=len(links), n_owned=n_owned, n_shadowed=n_shadowed)
    assert out["n_fragments"] == kept - outside == sum(T.values())
    for k in REC_KEYS:
        out[k] = np.array(R[k], np.uint32)
    rows = [(a, b) + tuple(v) for (a, b), v in sorted(links.items()) if v[0] >= min_pairs]
    for j, k in enumerate(LINK_KEYS):
        out[k] = np.array([x[j] for x in rows], np.uint64 if k == "len_sum" else np.uint32)
    return out


def same(got, want):
    """Field by field; returns the first field that differs, or None."""
    for k in TOTALS:
        if int(got[k]) != int(want[k]):
            return k
    for k in REC_KEYS + LINK_KEYS:
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            return k
    return None


def identity(l):
    return int(l["n_unowned"]) + int(l["n_inside"]) + int(l["n_open"]) + int(l["n_link_pairs"]) == int(l["n_fragments"]) == int(l["n_kept"]) - int(l["n_outside"])


def tsv(l, unit):
    """Expected text of the links of l."""
    return b"".join(b"p%d_%d\tp%d_%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((unit, a, unit, b) + tuple(int(v) for v in rest))
                    for a, b, *rest in zip(*(np.asarray(l[k]).tolist() for k in LINK_KEYS)))
