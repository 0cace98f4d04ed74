"""An independent model of the walk preparation (agx_core.h "walk preparation"; agx_k_assign_aid, agx_k_emit_alive, agx_k_special_bits,
agx_k_special_emit, agx_k_fetch_records in agx_kernels.hip): the walk graph a unit must hand to the host walk, worked out with numpy from the
oracle's canonical graph dump (harness.run_oracle(graph=True)) and the coverage threshold.  It is written from the prose of that comment block and
the reference lines it cites, and calls none of the lane functions:

  alive      a node survives the prune iff it lies on a contig or has the coverage (AG:1904-1918)
  walk ids   the first alive variant of position X is id X; the further alive variants follow from n_pos on, position-major, in variant order
  base       the consensus, max(A, C, G, T, N) with ties in that order, or the position's own base where nothing voted (AG:1944-1952, 1997-2001)
  meta       ABSENT (and base 'N') on main ids without an alive node; ANY on main ids whose position holds a variant, pruned or not (AG:2428);
             CONTIG where contigOffset != -1 (AG:2004); SIDE on main ids with further alive variants; CONT where the node has exactly one alive
             successor, that successor is id + 1, and its out-degree BEFORE pruning is at most 4 (the spill flag is set while the edges are built)
  special    side ids; ids without CONT; ids behind one without CONT; id 0; alive targets of ids without CONT and the id in front of each; main
             ids of positions where a conti-mer chain ends and the id in front of each; never an ABSENT id.  (Why the id in FRONT of a chain end: a
             walk that leaves a chain steps back onto the k-mer graph at the chain's last position and marks the node there traversed, AG:2093-2136,
             exactly as a jump marks its target; a forced run that comes along later must stop in front of that node, AG:2020-2046, so the walk needs
             the record of the id before it, for the same reason as before a jump's target.)
  records    per id the alive successors as a set, mate offset, position and k-mer string length
  hops       per position with exactly one conti-mer that has a next (AG:2047-2057): the bases appended and the landing position

mismatch() compares a dump (Unit.walk_graph / hostsim.sim.run(walk=True)["walk"]) with the model.  Its only freedoms: the order of a record's
successor slots, which successors of a spilled node sit in the slots and which on the overflow list, and NONE/NONE or repeated overflow entries.
"""
import numpy as np

NONE = 0xFFFFFFFF
CONT, CONTIG, SIDE, ANY, ABSENT = 1, 2, 4, 8, 128
MAXE = 4


def build(g, coverage, sparse_min=False):
    """g: the oracle's graph dump.  Returns the expected walk graph as a dict of numpy arrays (see mismatch for what is compared)."""
    n_pos, nn = int(g["n_pos"]), int(g["n_nodes"])
    ns = g["node_start"].astype(np.int64)
    per_pos = np.diff(ns)
    pos_of = np.repeat(np.arange(n_pos, dtype=np.int64), per_pos)
    key, cnt = g["node_key"].astype(np.int64), g["node_cnt"].astype(np.int64)
    alive = (key[:, 0] != NONE) | (cnt[:, 0] >= coverage) if nn else np.zeros(0, bool)
    before = np.concatenate(([0], np.cumsum(alive)))                     # alive nodes in front of node v
    rank = before[:nn] - before[ns[pos_of]] if nn else np.zeros(0, np.int64)      # alive variants of the same position in front of v
    is_main, is_side = alive & (rank == 0), alive & (rank > 0)
    n_side = int(is_side.sum())
    n_ids = n_pos + n_side
    aid = np.full(nn, -1, np.int64)
    aid[is_main] = pos_of[is_main]
    aid[is_side] = n_pos + np.arange(n_side)                            # node order is position-major, variant order
    node_of = np.full(n_ids, -1, np.int64)
    node_of[aid[alive]] = np.nonzero(alive)[0]
    alive_at = np.bincount(pos_of[alive], minlength=n_pos) if nn else np.zeros(n_pos, np.int64)

    votes = cnt[:, 1:6]
    ref = np.frombuffer(g["pos_nuc"], dtype=np.uint8)
    base = np.where(votes.sum(axis=1) == 0, ref[pos_of], np.frombuffer(b"ACGTN", dtype=np.uint8)[np.argmax(votes, axis=1)]) if nn else np.zeros(0, np.uint8)

    # edges in walk ids, pruned ends dropped; out-degree before pruning
    es = g["edge_start"].astype(np.int64)
    e_src = np.repeat(np.arange(nn, dtype=np.int64), np.diff(es))
    e_dst = g["edge_dst"].astype(np.int64)
    deg_all = np.diff(es)
    keep = alive[e_src] & alive[e_dst] if len(e_src) else np.zeros(0, bool)
    a_src, a_dst = aid[e_src[keep]], aid[e_dst[keep]]
    pairs = np.unique((a_src << 32) | a_dst)
    a_src, a_dst = pairs >> 32, pairs & 0xFFFFFFFF
    deg_alive = np.bincount(a_src, minlength=n_ids)
    only = np.full(n_ids, -1, np.int64)
    only[a_src] = a_dst                                                 # (meaningful where deg_alive == 1)
    spilled = np.zeros(n_ids, bool)
    spilled[aid[alive]] = deg_all[alive] > MAXE

    ids = np.arange(n_ids, dtype=np.int64)
    has = node_of >= 0
    v = np.where(has, node_of, 0)
    cont = has & (deg_alive == 1) & (only == ids + 1) & ~spilled
    meta = np.zeros(n_ids, np.int64)
    meta[cont] |= CONT
    meta[has & (key[v, 1] != NONE)] |= CONTIG
    main = ids < n_pos
    meta[:n_pos][(alive_at >= 2)] |= SIDE
    meta[:n_pos][per_pos > 0] |= ANY
    meta[main & ~has] |= ABSENT
    meta[main & ~has] &= (ABSENT | ANY)
    s = np.full(n_ids, ord("N"), np.uint8)
    s[has] = base[v[has]]

    mark = np.zeros(n_ids + 1, bool)
    mark[a_dst[~cont[a_src]]] = True
    mark[np.nonzero(g["chain_end"])[0]] = True
    special = ~main & has
    if not sparse_min:
        prev_cont = np.concatenate(([False], cont[:-1]))
        special |= main & has & (~cont | (ids == 0) | ~prev_cont | mark[:n_ids] | mark[1:])
    n_words = n_ids // 64 + 1
    padded = np.zeros(n_words * 64, bool)
    padded[:n_ids] = special
    bits = (padded.reshape(n_words, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    per_word = padded.reshape(n_words, 64).sum(axis=1)
    rank_w = np.concatenate(([0], np.cumsum(per_word)[:-1]))

    xpos = ids.copy()
    xpos[has] = pos_of[v[has]]
    return {"n_pos": n_pos, "n_ids": n_ids, "n_special": int(special.sum()), "meta": meta.astype(np.uint8), "str": s.tobytes(),
            "side_xpos": xpos[n_pos:].astype(np.uint32), "special": special, "sp_bits": bits, "sp_rank": rank_w.astype(np.uint32),
            "cont": cont, "mark": mark, "spilled": spilled, "has": has, "edges": pairs,
            "off0": np.where(has, key[v, 5], NONE).astype(np.uint32), "xpos": xpos.astype(np.uint32),
            "slen": np.where(has, g["node_slen"].astype(np.int64)[v], 0).astype(np.uint32),
            "per_pos": per_pos, "alive_at": alive_at, "cm_count": g["cm_count"],
            "hop_off": g["hop_off"], "hop_len": g["hop_len"], "hop_end": g["hop_end"], "hop_str": g["hop_str"]}


def slen_of(recs):
    return (recs["sref_qlen"] >> 16) & 0x7FFF


def _records_mismatch(m, ids, recs, ovf, what):
    """The records `recs` of the walk ids `ids` (ascending) against the model: position, mate offset, k-mer string length, successor sets."""
    for f, want in (("xpos", m["xpos"][ids]), ("off0", m["off0"][ids])):
        if not np.array_equal(recs[f], want):
            i = int(np.nonzero(recs[f] != want)[0][0])
            return "%s: %s of id %d is %d, expected %d" % (what, f, ids[i], recs[f][i], want[i])
    if not np.array_equal(slen_of(recs), m["slen"][ids]):
        i = int(np.nonzero(slen_of(recs) != m["slen"][ids])[0][0])
        return "%s: k-mer string length of id %d is %d, expected %d" % (what, ids[i], slen_of(recs)[i], m["slen"][ids][i])
    nx = recs["next"].astype(np.int64)
    used = nx != NONE
    if len(nx) and (used[:, 1:] & ~used[:, :-1]).any():
        return "%s: a successor slot behind an empty one (id %d)" % (what, ids[np.nonzero((used[:, 1:] & ~used[:, :-1]).any(axis=1))[0][0]])
    slot = (np.repeat(ids, MAXE).reshape(-1, MAXE)[used] << 32) | nx[used]
    if len(np.unique(slot)) != len(slot):
        return "%s: a successor listed twice in one record" % what
    o = ovf.astype(np.int64)
    o = o[(o[:, 0] != NONE) & np.isin(o[:, 0], ids)]
    got = np.unique(np.concatenate((slot, (o[:, 0] << 32) | o[:, 1])))
    want = m["edges"][np.isin(m["edges"] >> 32, ids)]
    if not np.array_equal(got, want):
        d = np.setxor1d(got, want)[0]
        return "%s: successor sets differ first at edge %d -> %d (%s)" % (what, d >> 32, d & 0xFFFFFFFF, "missing" if d in want else "surplus")
    return None


def mismatch(m, d, records=True):
    """First difference between the model m (build) and a walk-graph dump d, or None.  records=False leaves out d["all_node"] (a dump without it)."""
    for k in ("n_pos", "n_ids"):
        if m[k] != d[k]:
            return "%s: %d, expected %d" % (k, d[k], m[k])
    n_pos, n_ids = m["n_pos"], m["n_ids"]
    ids = np.arange(n_ids, dtype=np.int64)
    for k in ("meta", "side_xpos", "sp_bits", "sp_rank"):
        if len(d[k]) != len(m[k]) or not np.array_equal(d[k], m[k]):
            i = int(np.nonzero(np.asarray(d[k]) != np.asarray(m[k]))[0][0]) if len(d[k]) == len(m[k]) else -1
            return "%s differs first at %d: %s, expected %s" % (k, i, d[k][i] if i >= 0 else len(d[k]), m[k][i] if i >= 0 else len(m[k]))
    if d["str"] != m["str"]:
        i = next(i for i in range(n_ids) if d["str"][i] != m["str"][i])
        return "str differs first at id %d: %r, expected %r" % (i, d["str"][i:i + 1], m["str"][i:i + 1])
    if d["n_special"] != m["n_special"] or len(d["sp_node"]) != m["n_special"] or len(d["sp_hop"]) != m["n_special"]:
        return "n_special: %d (%d records, %d hop entries), expected %d" % (d["n_special"], len(d["sp_node"]), len(d["sp_hop"]), m["n_special"])
    ovf = d["ovf"]
    o = ovf.astype(np.int64)
    half = (o[:, 0] == NONE) != (o[:, 1] == NONE)
    if half.any():
        return "overflow entry %d names one end only" % int(np.nonzero(half)[0][0])
    o = o[o[:, 0] != NONE]
    if len(o):
        if (o >= n_ids).any():
            return "an overflow entry names an id beyond the walk graph"
        if not m["spilled"][o[:, 0]].all():
            return "overflow entry from id %d, whose node did not spill" % o[~m["spilled"][o[:, 0]]][0, 0]
        if not np.isin((o[:, 0] << 32) | o[:, 1], m["edges"]).all():
            return "an overflow entry is not an edge between alive nodes"
    sp = ids[m["special"]]
    bad = _records_mismatch(m, sp, d["sp_node"], ovf, "sparse table")
    if bad:
        return bad
    # hop entries, by what they append and where they land
    x = m["xpos"][sp].astype(np.int64)
    want_len = np.where(m["cm_count"][x] == 1, m["hop_len"][x], 0)
    h = d["sp_hop"]
    if not np.array_equal(h["len"], want_len):
        i = int(np.nonzero(h["len"] != want_len)[0][0])
        return "hop of id %d (position %d): %d bases, expected %d" % (sp[i], x[i], h["len"][i], want_len[i])
    for i in np.nonzero(want_len)[0]:
        so, n, xx = int(h["str_off"][i]), int(h["len"][i]), int(x[i])
        if so + n > len(d["chain_str"]):
            return "hop of id %d reads beyond chain_str" % sp[i]
        if h["end_pos"][i] != m["hop_end"][xx] or d["chain_str"][so:so + n] != m["hop_str"][int(m["hop_off"][xx]):int(m["hop_off"][xx]) + n]:
            return "hop of id %d (position %d) appends other bases or lands on %d, expected %d" % (sp[i], xx, h["end_pos"][i], m["hop_end"][xx])
    if records:
        if d.get("all_node") is None or len(d["all_node"]) != n_ids:
            return "no full record table in the dump"
        bad = _records_mismatch(m, ids, d["all_node"], ovf, "fetch path")
        if bad:
            return bad
        a = d["all_node"][~m["has"]]
        if len(a) and ((a["next"] != NONE).any() or (a["sref_qlen"] != 0).any() or (a["sref_slot"] != 0).any()):
            return "fetch path: the record of an absent id is not empty"
    return None


def same_bits(a, b):
    """First difference between two dumps in every field that is defined bit for bit (all but slot order, spill choice, overflow order, and the read a k-mer string is taken from), or None."""
    for k in ("n_pos", "n_ids", "n_special", "str"):
        if a[k] != b[k]:
            return k
    for k in ("meta", "side_xpos", "sp_bits", "sp_rank"):
        if not np.array_equal(a[k], b[k]):
            return k
    for t in ("sp_node", "all_node"):
        if (a.get(t) is None) != (b.get(t) is None):
            return t
        if a.get(t) is not None:
            for f in ("off0", "xpos"):
                if not np.array_equal(a[t][f], b[t][f]):
                    return t + "." + f
            if not np.array_equal(slen_of(a[t]), slen_of(b[t])):
                return t + ".slen"
    if not np.array_equal(a["sp_hop"]["len"], b["sp_hop"]["len"]):
        return "sp_hop.len"
    on = a["sp_hop"]["len"] != 0
    if not np.array_equal(a["sp_hop"]["end_pos"][on], b["sp_hop"]["end_pos"][on]) or not np.array_equal(a["sp_hop"]["str_off"][on], b["sp_hop"]["str_off"][on]) or a["chain_str"] != b["chain_str"]:
        return "sp_hop"
    return None
