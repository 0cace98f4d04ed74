"""A plain reference of the unitig export and of its id map, over dicts and lists: the alive nodes of a window at a threshold, their distinct edges,
degrees, every head followed along its single successors, the bases, the coverage sums and the sorted links.  It shares no code with tests/unitig_model.py,
tests/unitig_region_model.py or tests/path_model.py: tests/test_unitig_cases.py holds those three against it on units they were never run on."""
NONE = 0xFFFFFFFF


def unitigs(g, lo, hi, cov, ref):
    """(table with the fields of Unit.unitigs(), {canonical node: (segment, rank)}) of positions [lo, hi) at threshold cov."""
    ns, es, dst = (g[k].tolist() for k in ("node_start", "edge_start", "edge_dst"))
    key, cnt = g["node_key"].reshape(-1, 6).tolist(), g["node_cnt"].reshape(-1, 6).tolist()
    alive = {}                                              # node -> (position, variant), in (position, variant) order
    for x in range(lo, hi):
        for v in range(ns[x + 1] - ns[x]):
            if key[ns[x] + v][0] != NONE or cnt[ns[x] + v][0] >= cov:
                alive[ns[x] + v] = (x, v)
    succ, pred = {i: set() for i in alive}, {i: set() for i in alive}
    for i in alive:
        for d in dst[es[i]:es[i + 1]]:
            if d in alive:
                succ[i].add(d)
                pred[d].add(i)

    def step(i):                                            # the node behind i in its segment, or None
        if len(succ[i]) != 1:
            return None
        d = next(iter(succ[i]))
        return d if len(pred[d]) == 1 and d != i else None
    entered = {step(i) for i in alive} - {None}
    heads = [i for i in alive if i not in entered]
    seg_of, place, chains = {}, {}, []
    for s, h in enumerate(heads):
        chain, i = [], h
        while i is not None:
            place[i] = (s, len(chain))
            chain.append(i)
            i = step(i)
        seg_of[h] = s
        chains.append(chain)
    assert len(place) == len(alive), "a cycle of internal edges"
    seq = bytearray()
    for chain in chains:
        for i in chain:
            votes = cnt[i][1:6]
            seq.append(ref[alive[i][0]] if max(votes) == 0 else b"ACGTN"[votes.index(max(votes))])
    links = sorted((s, seg_of[d]) for s, chain in enumerate(chains) for d in succ[chain[-1]])      # (a chain ends where no step goes on: every successor of its last node is a head)
    off = [0]
    for chain in chains:
        off.append(off[-1] + len(chain))
    t = {"head_pos": [alive[h][0] for h in heads], "head_var": [alive[h][1] for h in heads], "n_nodes": [len(c) for c in chains],
         "last_pos": [alive[c[-1]][0] for c in chains], "coverage": [sum(cnt[i][0] for i in c) for c in chains], "seq_off": off, "seq": bytes(seq),
         "link_from": [a for a, _ in links], "link_to": [b for _, b in links]}
    return t, place


def id_map(g, coverage, lo, hi, cov, ref):
    """The runs of walk ids (of a unit built at `coverage`) whose nodes are in the export of [lo, hi) at cov: the first alive variant of position x is id x, the
    further ones follow from n_pos on, position by position."""
    ns = g["node_start"].tolist()
    key, cnt = g["node_key"].reshape(-1, 6).tolist(), g["node_cnt"].reshape(-1, 6).tolist()
    n_pos = len(ns) - 1
    place = unitigs(g, lo, hi, cov, ref)[1]
    node_of, side = {}, []
    for x in range(n_pos):
        live = [i for i in range(ns[x], ns[x + 1]) if key[i][0] != NONE or cnt[i][0] >= coverage]
        if live:
            node_of[x] = live[0]
            side += live[1:]
    for j, i in enumerate(side):
        node_of[n_pos + j] = i
    runs, prev = [], None                                   # prev: (segment, rank) of the id in front, if it is in the export
    for a in range(n_pos + len(side)):
        e = place.get(node_of.get(a))
        if e is not None:
            if prev is not None and a != n_pos and e == (prev[0], prev[1] + 1):
                runs[-1][1] = a
            else:
                runs.append([a, a, e[0], e[1]])
        prev = e
    return {"n_pos": n_pos, "n_ids": n_pos + len(side), "id_first": [r[0] for r in runs], "id_last": [r[1] for r in runs], "seg": [r[2] for r in runs],
            "rank_first": [r[3] for r in runs]}
