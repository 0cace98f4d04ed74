"""Edge support, the reference's way: how many events name each edge of a unit's graph.

Plain Python / numpy; nothing of the project is imported.  An EVENT is one call of update_kmer in the oracle's update_genome_with_reads
(oracle/agx_oracle.cpp; AG:1635-1870): per kept hit the two mates' position sets are laid out read index by read index and the loop over the indices
i < L - k makes the calls — the ordinary and deletion arm (the next index is aligned), and the read-insertion arm, which looks for the next aligned
index r and either steps to it directly (it lies on P + 1) or walks there through a chain of events without mate positions.  An event (P, N, P0, N0)
builds its candidate keys {conti-mers of P | none} x {conti-mers of P0 | none} (P-major), resolves each to the first compatible variant of the FINAL
bucket — the oracle's node_key table — and likewise at N; it names every pair (s, d) of the two sets of variants that passes the contig-consistency
test of AG:1602-1615, each pair once.

Inputs: the front of a unit in file order (hostsim sim.run(..., front=True)["front"]: dhit, runs, cm_start, cm — the position sets follow from the
derived records' runs; a_runs is ignored where both run counts are 0) and the oracle's graph dump (H.run_oracle(..., graph=True)["graph"]).
The events of all hits are collected first and resolved in batches (numpy), variant by variant in bucket order: the rule is the oracle's, only the
loop over events is turned inside out.
"""
import numpy as np

NONE = 0xFFFFFFFF
HF_SKIP = 2
EP25 = 25


def position_set(t0, first_run, n_runs, runs, L):
    """positionSets[hit] of one mate: the reference offset of every read index, NONE where the index is not aligned."""
    if n_runs == 0:
        return np.arange(t0, t0 + L, dtype=np.int64)
    p = np.full(L, NONE, np.int64)
    for r in runs[first_run:first_run + n_runs]:
        q, t, n = int(r["q"]), int(r["t"]), int(r["n"])
        p[q:q + n] = np.arange(t, t + n)
    return p


def events_of_hit(pa, pb, k):
    """The update_kmer calls of one hit as rows (P, N, P0, N0): the loop of update_genome_with_reads over the read indices."""
    L = len(pa)
    lim = L - k
    if lim <= 0:
        return np.zeros((0, 4), np.int64)
    if (pa[:lim + 1] != NONE).all():      # every index up to lim is aligned: the loop only ever takes its last arm
        return np.stack([pa[:lim], pa[1:lim + 1], pb[:lim], pb[1:lim + 1]], axis=1)
    out = []
    i = 0
    while i < lim:
        if pa[i] == NONE:
            i += 1
            continue
        P, P0 = int(pa[i]), int(pb[i])
        Nx, N0 = int(pa[i + 1]), int(pb[i + 1])
        if Nx == NONE:                    # insertion in the read
            for r in range(i + 2, L):
                if pa[r] == NONE:
                    continue
                Nx, N0 = int(pa[r]), int(pb[r])
                if Nx == P + 1:
                    out.append((P, Nx, P0, N0))
                else:                     # next to a gap of the reference: a chain of events without mate positions
                    out.append((P, P + 1, P0, NONE))
                    c = P + 1
                    while c < Nx - 1:
                        out.append((c, c + 1, NONE, NONE))
                        c += 1
                    out.append((c, c + 1, NONE, N0))
                i = r - 1
                break
        else:                             # deletion in the read, and the ordinary case
            out.append((P, Nx, P0, N0))
        i += 1
    return np.array(out, np.int64).reshape(-1, 4)


def events(front, k):
    """All events of the unit, hit by hit in file order: an [n, 4] array of (P, N, P0, N0)."""
    runs, rows = front["runs"], []
    for d in front["dhit"]:
        if int(d["flags"]) & HF_SKIP:
            continue
        L = int(d["len"])
        pa = position_set(int(d["a_t0"]), int(d["a_runs"]), int(d["a_nruns"]), runs, L)
        pb = position_set(int(d["b_t0"]), int(d["b_runs"]), int(d["b_nruns"]), runs, L)
        rows.append(events_of_hit(pa, pb, k))
    return np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)


def _clause_ab(ac, ao, bc, bo, win):
    """AG:1293-1312: true unless both ids are set and equal and the offsets lie further apart than win"""
    return (ac == NONE) | (bc == NONE) | (ac != bc) | (np.abs(ao - bo) <= win)


def _clause_c(ao, bo, win):
    return (ao == NONE) | (bo == NONE) | (np.abs(ao - bo) <= win)


def _variants(X, X0, graph, cm_start, cm, iv):
    """For events at positions X with mate positions X0: rows (event, variant) — the distinct variants the candidate keys resolve to."""
    n_pos = int(graph["n_pos"])
    ns = graph["node_start"].astype(np.int64)
    key = graph["node_key"].astype(np.int64)
    cms = cm_start.astype(np.int64)
    cid_all, coff_all = cm["cid"].astype(np.int64), cm["coff"].astype(np.int64)
    assert ((X >= 0) & (X < n_pos)).all() and ((X0 == NONE) | (X0 < n_pos)).all(), "an event beyond the unit"
    has0 = X0 != NONE
    x0 = np.where(has0, X0, 0)
    nx = cms[X + 1] - cms[X]
    n0 = np.where(has0, cms[x0 + 1] - cms[x0], 0)
    mx, m0 = np.maximum(nx, 1), np.maximum(n0, 1)
    ncand = mx * m0
    ev = np.repeat(np.arange(len(X)), ncand)
    j = np.arange(len(ev)) - np.repeat(np.cumsum(ncand) - ncand, ncand)
    i1, i0 = j // m0[ev], j % m0[ev]                      # P-major
    at1, at0 = np.minimum(cms[X[ev]] + i1, max(len(cid_all) - 1, 0)), np.minimum(cms[x0[ev]] + i0, max(len(cid_all) - 1, 0))
    if len(cid_all) == 0:
        cid_all, coff_all = np.full(1, NONE, np.int64), np.full(1, NONE, np.int64)
    k_cid = np.where(nx[ev] > 0, cid_all[at1], NONE)
    k_coff = np.where(nx[ev] > 0, coff_all[at1], NONE)
    k_cid0 = np.where(n0[ev] > 0, cid_all[at0], NONE)
    k_coff0 = np.where(n0[ev] > 0, coff_all[at0], NONE)
    k_off0 = X0[ev]
    k_chr0 = np.where(has0[ev], 0, NONE)
    # first compatible variant, bucket order
    base, cnt = ns[X[ev]], ns[X[ev] + 1] - ns[X[ev]]
    found = np.full(len(ev), -1, np.int64)
    open_ = np.arange(len(ev))
    v = 0
    while len(open_):
        open_ = open_[cnt[open_] > v]
        if not len(open_):
            break
        node = base[open_] + v
        nk = key[node]
        ok = _clause_ab(k_cid[open_], k_coff[open_], nk[:, 0], nk[:, 1], EP25) & _clause_ab(k_cid0[open_], k_coff0[open_], nk[:, 2], nk[:, 3], 2 * iv + EP25) & \
            ((k_chr0[open_] == NONE) | (nk[:, 4] == NONE) | ((k_chr0[open_] == nk[:, 4]) & (np.abs(k_off0[open_] - nk[:, 5]) <= 2 * iv + EP25)))
        found[open_[ok]] = node[ok]
        open_ = open_[~ok]
        v += 1
    keep = found >= 0
    pairs = np.unique(np.stack([ev[keep], found[keep]], axis=1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    return pairs[:, 0], pairs[:, 1]


def support(front, graph, k, iv):
    """The support of every edge of the oracle's graph.  Returns a dict:
    n_events, n_contributions; edge_start / edge_dst: the oracle's edges sorted per node (agx_unit_graph's numbering); edge_cnt: their support;
    off_graph: contributions that name a pair that is no edge (must be 0); pairs: {(src, dst): count}."""
    E = events(front, k)
    nn = int(graph["n_nodes"])
    es = graph["edge_start"].astype(np.int64)
    owner = np.repeat(np.arange(nn, dtype=np.int64), np.diff(es))
    order = np.lexsort((graph["edge_dst"].astype(np.int64), owner))
    edge_dst = graph["edge_dst"].astype(np.int64)[order]
    edge_code = owner * (nn + 1) + edge_dst                 # ascending
    out = {"n_events": len(E), "edge_start": graph["edge_start"].astype(np.uint32), "edge_dst": edge_dst.astype(np.uint32)}
    if not len(E):
        out.update(n_contributions=0, edge_cnt=np.zeros(len(edge_dst), np.uint32), off_graph=0, pairs={})
        return out
    ev_s, id_s = _variants(E[:, 0], E[:, 2], graph, front["cm_start"], front["cm"], iv)
    ev_d, id_d = _variants(E[:, 1], E[:, 3], graph, front["cm_start"], front["cm"], iv)
    # S x D per event
    cd = np.bincount(ev_d, minlength=len(E))
    start_d = np.cumsum(cd) - cd
    rep = cd[ev_s]
    s_rows = np.repeat(np.arange(len(ev_s)), rep)
    kth = np.arange(len(s_rows)) - np.repeat(np.cumsum(rep) - rep, rep)
    src, dst = id_s[s_rows], id_d[start_d[ev_s[s_rows]] + kth]
    key = graph["node_key"].astype(np.int64)
    a, b = key[src], key[dst]
    allowed = _clause_ab(b[:, 0], b[:, 1], a[:, 0], a[:, 1], EP25) & _clause_ab(b[:, 2], b[:, 3], a[:, 2], a[:, 3], 2 * iv + EP25)
    code = (src * (nn + 1) + dst)[allowed]
    uniq, cnt = np.unique(code, return_counts=True)
    at = np.searchsorted(edge_code, uniq)
    hit = (at < len(edge_code)) & (edge_code[np.minimum(at, max(len(edge_code) - 1, 0))] == uniq) if len(edge_code) else np.zeros(len(uniq), bool)
    edge_cnt = np.zeros(len(edge_code), np.int64)
    edge_cnt[at[hit]] = cnt[hit]
    out.update(n_contributions=int(cnt.sum()), edge_cnt=edge_cnt.astype(np.uint32), off_graph=int(cnt[~hit].sum()),
               pairs={(int(c // (nn + 1)), int(c % (nn + 1))): int(n) for c, n in zip(uniq, cnt)})
    return out


def edge_support_of(sup, src, dst):
    """The support of edge src -> dst (canonical ids) in what support() or Unit.edge_support() returns; None if it is no edge."""
    lo, hi = int(sup["edge_start"][src]), int(sup["edge_start"][src + 1])
    at = lo + int(np.searchsorted(sup["edge_dst"][lo:hi], dst))
    return int(sup["edge_cnt"][at]) if at < hi and int(sup["edge_dst"][at]) == dst else None
