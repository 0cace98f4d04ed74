"""Hand-made units that pin the unitig export (agx_unitig.hip; export_body / region_export, agx_export.cpp; the id map behind --graphPaths) arm by arm.

The units are lean_units.Unit's / walk_units.WUnit's written by walk_units.write_unit, so the CPU twin (tests/test_unitig_cases.py) and the GPU file
(tests/test_gpu_unitig_cases.py) build exactly the same inputs.  What is correct is decided by tests/unitig_model.py, tests/unitig_region_model.py and
tests/path_model.py on the oracle's graph (and those by the plain reference of tests/unitig_plain.py); nothing here works out expected output.

What this module adds is the PIECE MODEL: in the region export a node's id is its rank among the kept nodes of [lo, hi) at the threshold in (position, variant)
order (agx_k_utr_compact), so the oracle's graph fixes every id, every lane (id % 64), every 256-thread block (id // 256), every piece (ut_window_of / ut_cut:
a run of internal edges id -> id + 1 that lane 63 never continues), the number of pieces np, the rounds of pointer jumping and the chain of pieces of every
segment.  piece_model() restates that with numpy and imports nothing of the project.  Each case names its windows (lo, hi, threshold) and its arms, predicates on the
piece model of one named window (or on the executor's overflow dump, hostsim.sim.run(..., edges=True)["ovf"], for membership of the overflow list); check_arms()
asserts them, so a case cannot silently stop reaching its arm.  Moving lo moves a feature of the unit to any lane one likes.

The whole export works on slots, which no hook shows: it gets the same units and equality with the model and with the region form, and no arms of its own.

Not as the issue's table has it:
  branch_lanes  edge_units' single -> multi recipe (case_boundary) makes no branch: the one read that steps from X to X + 1 joins one of X + 1's variants, so X keeps a
                single successor and the other variant starts a strand of its own.  The branch here is a deletion read (dele(X, [1]): X -> X + 1 and X -> X + 2), which makes
                X a tail with two links, X + 1 a one-node segment and X + 2 a head where the strands merge; the single -> multi -> single stretch stands further along the
                same strand (MULTI), where its second variant's head and tail are looked at.
  islands       a one-node island cannot be written through the loaders (a read aligned over fewer bases than the identity filter admits is dropped, and a read's last
                arrival has no coverage of its own): the one-node segments without links come from windows that cut one node off an island's end.
  map_edges     the fix-up `i == n_main` of agx_k_idm_flags / agx_k_idm_runs (a run never holds a main id and a side id) cannot change a result: the window's last main id
                is the last position's first variant, and the node behind it in a segment lies at a later position, outside the window, so the first side id never continues
                it.  What is reached is the layout around it: the main run ends on id n_main - 1, a side run starts at n_main, with n_main on and off a multiple of 64.
  straight      rounds of both parities are reached, but the parity alone cannot show in a result: ceil(log2 np) + 1 rounds are one more than a chain of np pieces needs, so
                the buffer of the round before holds the same ancestors and offsets.  What the chains of np pieces hold is the number of rounds itself.
  strands_2     inside the doubled stretch np is even (two nodes per position, every node a piece); the odd values 4 095 and 4 097 come from windows that start 64 positions
                in front of it (the lead-in's 64 nodes are one piece, lane 63 does not link).
"""
import numpy as np

import lean_units as LU
from edge_units import OFF, SEP, cover, dele, end_at, span, start_at, variants
from lean_units import Unit, pair

NONE = 0xFFFFFFFF
HIGH = 1 << 30          # a coverage no read pile reaches: only contig nodes survive


class Pieces:
    """What piece_model returns; ids are the region export's local ids."""


def piece_model(graph, lo, hi, cov):
    """The plumbing of the region export of positions [lo, hi) at threshold cov, from a canonical graph dump.  Fields: kept (nodes), node / pos / var / cnt per id,
    outdeg, indeg, nxt (-1: a tail), haspred, link, starts (first id of every piece), np, piece_of, p_len, heads, tails, lane, block, chains (per segment, in head order,
    its piece ids from the head's on), seg_of, rounds, links ((tail id, head id), distinct)."""
    ns = np.asarray(graph["node_start"], dtype=np.int64)
    n_pos, nn = len(ns) - 1, int(ns[-1])
    assert 0 <= lo <= hi <= n_pos
    pos_all = np.repeat(np.arange(n_pos, dtype=np.int64), np.diff(ns))
    key0 = np.asarray(graph["node_key"], dtype=np.int64).reshape(-1, 6)[:, 0]
    cnt = np.asarray(graph["node_cnt"], dtype=np.int64).reshape(-1, 6)
    kept = (pos_all >= lo) & (pos_all < hi) & ((key0 != NONE) | (cnt[:, 0] >= cov))      # unitig_region_model.region_graph's rule
    node = np.nonzero(kept)[0]
    n = len(node)
    lid = np.full(nn, -1, np.int64)
    lid[node] = np.arange(n)
    es = np.asarray(graph["edge_start"], dtype=np.int64)
    src = np.repeat(np.arange(nn, dtype=np.int64), np.diff(es))
    dst = np.asarray(graph["edge_dst"], dtype=np.int64)
    both = kept[src] & kept[dst]
    code = np.unique(lid[src[both]] * max(n, 1) + lid[dst[both]])          # an edge listed twice counts once
    s, d = code // max(n, 1), code % max(n, 1)
    outdeg, indeg = np.bincount(s, minlength=n), np.bincount(d, minlength=n)
    internal = (outdeg[s] == 1) & (indeg[d] == 1)
    nxt = np.full(n, -1, np.int64)
    nxt[s[internal]] = d[internal]
    haspred = np.zeros(n, bool)
    haspred[d[internal]] = True
    ids = np.arange(n, dtype=np.int64)
    link = (nxt == ids + 1) & (ids % 64 != 63)                              # ut_window_of: lane 63 never links
    start = np.ones(n, bool)
    start[1:] = ~link[:-1]
    P = Pieces()
    P.lo, P.hi, P.cov, P.kept, P.node, P.pos, P.var, P.cnt = lo, hi, cov, n, node, pos_all[node], node - ns[pos_all[node]], cnt[node]
    P.outdeg, P.indeg, P.nxt, P.haspred, P.link = outdeg, indeg, nxt, haspred, link
    P.starts = np.nonzero(start)[0]
    P.np = len(P.starts)
    P.piece_of = np.cumsum(start) - 1
    P.p_len = np.bincount(P.piece_of, minlength=P.np)
    P.heads, P.tails = np.nonzero(~haspred)[0], np.nonzero(nxt < 0)[0]
    P.lane, P.block = ids % 64, ids // 256
    P.chains, P.seg_of = [], np.full(n, -1, np.int64)
    for g, h in enumerate(P.heads.tolist()):
        chain, p = [], int(P.piece_of[h])
        while True:
            chain.append(p)
            a = int(P.starts[p])
            P.seg_of[a:a + int(P.p_len[p])] = g
            t = int(nxt[a + int(P.p_len[p]) - 1])
            if t < 0:
                break
            assert start[t], "an internal edge that leaves a piece enters the middle of one"
            p = int(P.piece_of[t])
        P.chains.append(chain)
    assert (P.seg_of >= 0).all() and sum(len(c) for c in P.chains) == P.np
    P.rounds = 1
    while P.rounds < 32 and (1 << (P.rounds - 1)) < P.np:                   # ceil(log2 np) + 1: restated from export_body (agx_export.cpp)
        P.rounds += 1
    ext = ~internal
    P.links = sorted(zip(s[ext].tolist(), d[ext].tolist()))
    return P


def where(P, node_id):
    """'id, lane, block, piece' of a node of the piece model: what a failure message says about the first differing node."""
    p = int(P.piece_of[node_id])
    return "local id %d (position %d variant %d): lane %d, block %d, piece %d (ids %d..%d) of %d, segment %d" % (
        node_id, P.pos[node_id], P.var[node_id], node_id % 64, node_id // 256, p, P.starts[p], P.starts[p] + P.p_len[p] - 1, P.np, P.seg_of[node_id])


TABLE = ("head_pos", "head_var", "n_nodes", "last_pos", "coverage", "seq_off", "link_from", "link_to")


def table_mismatch(got, want):
    """First difference of two unitig tables (Unit.unitigs() or a model's: arrays or lists) as (field, index, text), or None."""
    for f in TABLE:
        a, b = np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)
        i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None)
        if i is not None:
            return f, i, "%s[%d] = %d, expected %d" % (f, i, a[i], b[i])
        if len(a) != len(b):
            return f, min(len(a), len(b)), "%s has %d entries, expected %d" % (f, len(a), len(b))
    a, b = bytes(got["seq"]), bytes(want["seq"])
    if a != b:
        i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        return "seq", i, "seq[%d] = %r, expected %r" % (i, a[i:i + 1], b[i:i + 1])
    return None


def node_of_entry(P, want, field, index):
    """The local id an entry of the expected table speaks about: a segment's head (its tail for last_pos), the tail of a link's segment, the node of a base; None beyond the table."""
    order = [int(P.starts[p]) + j for ch in P.chains for p in ch for j in range(int(P.p_len[p]))]      # ids in the order of seq
    segs = len(P.chains)
    if field == "seq":
        return order[index] if index < len(order) else None
    if field in ("link_from", "link_to"):
        g = int(np.asarray(want["link_from"])[index]) if index < len(want["link_from"]) else None
    else:
        g = min(index, segs - 1) if field == "seq_off" else index
    if g is None or not 0 <= g < segs:
        return None
    last = P.chains[g][-1]
    return int(P.heads[g]) if field in ("head_pos", "head_var", "n_nodes", "seq_off") else int(P.starts[last] + P.p_len[last] - 1)


def export_mismatch(case, ctx, w, got, want):
    """None, or what a failure says: the case, the window, the threshold, the first differing field and index, and where the piece model has that node."""
    x = table_mismatch(got, want)
    if x is None:
        return None
    P = ctx.pm(w)
    i = node_of_entry(P, want, x[0], x[1])
    return "%s: window [%d, %d) at threshold %d (kept %d, np %d, rounds %d): %s; %s" % (
        case.name, w[0], w[1], w[2], P.kept, P.np, P.rounds, x[2], where(P, i) if i is not None else "beyond the expected table")


RUNS = ("id_first", "id_last", "seg", "rank_first")


def map_shapes(m, lo, hi, side_xpos):
    """What an id map (Unit.unitigs(id_map=True)["id_map"] or a model's) of window [lo, hi) shows, in the window's ids (main id a is a - lo, the window's j-th side id is
    (hi - lo) + j: agx_k_idm_flags / agx_k_idm_runs take 64 of them per wavefront); side_xpos: the positions of the unit's side ids."""
    n, n_main = int(m["n_pos"]), hi - lo
    sx = np.asarray(side_xpos, dtype=np.int64)
    first, last = np.asarray(m["id_first"], dtype=np.int64), np.asarray(m["id_last"], dtype=np.int64)
    main = first < n
    side_lo = int((sx < lo).sum())
    wf = np.where(main, first - lo, n_main + first - n - side_lo)
    wl = wf + (last - first)
    out = set()
    if (main & (wf // 64 != wl // 64)).any():
        out.add("a run of main ids across a 64-id boundary")
    if ((~main) & (wf // 64 != wl // 64)).any():
        out.add("a run of side ids across a 64-id boundary")
    if main.any() and (~main).any() and wl[main].max() == n_main - 1 and wf[~main].min() == n_main:
        out.add("a run ends on the last main id and a side run starts at n_main")
    out.add("n_main is a multiple of 64" if n_main % 64 == 0 else "n_main is no multiple of 64")
    present = np.zeros(n_main + int(((sx >= lo) & (sx < hi)).sum()), bool)
    for a, b in zip(wf.tolist(), wl.tolist()):
        present[a:b + 1] = True
    if not present[:n_main].all():
        out.add("a main id without a node in the export")
    if not present[n_main:].all():
        out.add("a side id dead at the threshold")
    if (wl % 64 == 63).any() and (wf % 64 == 0).any():
        out.add("runs that end on lane 63 and start on lane 0")
    return out


class Case:
    def __init__(self, name, unit, windows, arms, coverage=1, iv=LU.IV, reprune=(), maps=(), edges=False, empty=(), support=False, map_want=None):
        """windows: [(lo, hi, threshold)], every one exported and compared; arms: [(description, window, fn(P, ctx) -> bool)], P the piece model of the window, which is
        one of `windows`; reprune: the thresholds the whole export is re-pruned to; maps: the windows (of `windows`) whose id map is compared, map_want: {window: what map_shapes must show of its id map}; edges: the arms read the
        executor's overflow dump (ctx.ovf: (source position, target position, listed again)); empty: the windows that may keep no node; support: the links' support is
        compared too."""
        self.name, self.unit, self.windows, self.arms, self.coverage, self.iv = name, unit, list(windows), list(arms), coverage, iv
        self.reprune, self.maps, self.edges, self.empty, self.support, self.map_want = tuple(reprune), list(maps), edges, list(empty), support, dict(map_want or {})


class Ctx:
    """A case's oracle graph (and the executor's run, where the case asks for it), with the piece model of every window made once."""

    def __init__(self, case, graph, sim_out=None):
        self.case, self.g, self.sim, self._pm = case, graph, sim_out, {}
        self.n_pos = int(graph["n_pos"])
        self.ref = bytes(graph["pos_nuc"])
        self.ovf = [(int(e["x"]), int(e["xs"]), int(e["again"])) for e in sim_out["ovf"]] if sim_out is not None else None

    def pm(self, w):
        if w not in self._pm:
            self._pm[w] = piece_model(self.g, *w)
        return self._pm[w]

    def widest(self):
        return max(self.case.windows, key=lambda w: (self.pm(w).kept, w[1] - w[0]))


def check_map_shapes(case, w, m, side_xpos):
    missing = case.map_want.get(w, set()) - map_shapes(m, w[0], w[1], side_xpos)
    assert not missing, "%s: the id map of window %s does not show: %s" % (case.name, w, sorted(missing))


def check_arms(case, ctx):
    assert case.arms, "%s: no arms" % case.name
    assert set(case.map_want) <= set(case.maps)
    assert set(case.maps) <= set(case.windows) and set(case.empty) <= set(case.windows) and len(set(case.windows)) == len(case.windows)
    for w in case.windows:
        assert w in case.empty or ctx.pm(w).kept > 0, "%s: window %s keeps no node" % (case.name, w)
    for w in case.empty:
        assert ctx.pm(w).kept == 0, "%s: window %s is not empty" % (case.name, w)
    for what, w, fn in case.arms:
        assert w in case.windows, "%s: %s: window %s is not exported" % (case.name, what, w)
        assert fn(ctx.pm(w), ctx), "%s: window %s: %s" % (case.name, w, what)


# ---- predicates --------------------------------------------------------------------------------------------------------------------------

def id_at(P, x, v=0):
    """local id of the node (x, v), -1 if it is not kept"""
    i = np.nonzero((P.pos == x) & (P.var == v))[0]
    return int(i[0]) if len(i) else -1


def seg_len(P, g):
    return int(P.p_len[P.chains[g]].sum())


def is_tail(P, i):
    return i >= 0 and P.nxt[i] < 0


def is_head(P, i):
    return i >= 0 and not P.haspred[i]


# ---- straight ----------------------------------------------------------------------------------------------------------------------------

S0 = 1024          # first position of the windows of `straight` (the strand runs from 960 to 2254)
STRAIGHT_KEPT = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
STRAIGHT_NP = {1: 1, 65: 2, 129: 3, 256: 4, 257: 5, 512: 8, 513: 9, 1024: 16, 1025: 17}


def case_straight():
    """One strand of single-variant positions: ids are positions, pieces are the 64-id groups: np on both sides of every power of two up to 16, rounds of both parities,
    one segment whose chain holds every piece."""
    wins = [(S0, S0 + n, 1) for n in STRAIGHT_KEPT]
    arms = [("kept = %d" % n, (S0, S0 + n, 1), lambda P, c, n=n: P.kept == n) for n in STRAIGHT_KEPT]
    for n, want in STRAIGHT_NP.items():
        arms.append(("np = %d, one segment of np pieces, every piece but the last 64 long" % want, (S0, S0 + n, 1),
                     lambda P, c, want=want: P.np == want and len(P.chains) == 1 and len(P.chains[0]) == want and (P.p_len[:-1] == 64).all()))
    arms.append(("rounds of both parities", wins[0], lambda P, c: {c.pm(w).rounds & 1 for w in wins} == {0, 1}))
    arms.append(("rounds = 1, 2, 3, 4, 5, 6", wins[0], lambda P, c: {c.pm(w).rounds for w in wins} == {1, 2, 3, 4, 5, 6}))
    return Case("straight", Unit(4096, cover(1000, 2200)), wins, arms, reprune=(3, 0))


# ---- strands -----------------------------------------------------------------------------------------------------------------------------

D2, E2 = 1160, 3455          # strands_2: the doubled stretch [D2, E2) (two variants per position); the first strand alone over [960, D2) and [E2, 3655)
D3, E3 = 1110, 1605          # strands_3: three variants per position


def own_pieces(P, lo, hi, jump):
    """every kept node of positions (lo, hi - 1) is a piece of its own whose internal edge goes `jump` ids on (the first strand's node at lo ends the lead-in's piece)"""
    m = (P.pos > lo) & (P.pos < hi - 1)
    ids = np.nonzero(m)[0]
    return m.any() and (P.p_len[P.piece_of[ids]] == 1).all() and (P.nxt[ids] == ids + jump).all()


def mixed_segment(P):
    """a segment made of pieces longer than 1 and of one-node pieces, its chain 256 pieces deep or more"""
    return any(len(ch) >= 256 and (P.p_len[ch] > 1).any() and (P.p_len[ch] == 1).sum() >= 255 for ch in P.chains)


def strands_unit():
    return Unit(8192, cover(1000, 3600) + cover(1200, 3400, OFF + SEP))


def case_strands_2():
    """Two strands that never touch over 2 296 positions, the first one alone in front of them and behind: in the doubled stretch every node is a piece of its own
    (nxt = id + 2), so np is the number of kept nodes: the scans under s_len / s_links (np + 1 elements in blocks of 4 096) at np = 4 094 .. 4 097, the scan under cntw
    at windows of 4 094 .. 4 097 positions, chains of more than 2 000 pieces."""
    w_np = {4094: (D2, D2 + 2047, 1), 4095: (D2 - 64, D2 + 2047, 1), 4096: (D2, D2 + 2048, 1), 4097: (D2 - 64, D2 + 2048, 1)}
    w_pos = [(500, 500 + n, 1) for n in (4094, 4095, 4096, 4097)]
    lead = (D2 - 100, D2 + 400, 1)
    both = (D2 - 100, E2 + 100, 1)
    wins = list(w_np.values()) + w_pos + [lead, both, (D2, D2 + 400, 1)]
    arms = [("np = %d" % n, w, lambda P, c, n=n: P.np == n) for n, w in w_np.items()]
    arms += [("a window of %d positions" % (w[1] - w[0]), w, lambda P, c: P.kept > 4097) for w in w_pos]
    arms += [("two segments of 400 nodes, 800 pieces, 798 internal edges id -> id + 2", (D2, D2 + 400, 1),
              lambda P, c: P.kept == 800 and P.np == 800 and int((P.nxt == np.arange(800) + 2).sum()) == 798 and [seg_len(P, g) for g in range(len(P.chains))] == [400, 400]),
             ("every node of the doubled stretch is a piece of its own", both, lambda P, c: own_pieces(P, D2, E2, 2)),
             ("a segment of long pieces and one-node pieces, 256 pieces deep", lead, lambda P, c: mixed_segment(P)),
             ("a lead-in and a lead-out around the doubled stretch in one segment", both,
              lambda P, c: any(P.p_len[ch[0]] > 1 and P.p_len[ch[-1]] > 1 and len(ch) > 2000 for ch in P.chains))]
    return Case("strands_2", strands_unit(), wins, arms, reprune=(2, 0))


def case_strands_3():
    """Three strands over 496 positions (nxt = id + 3), the first one alone in front and behind."""
    lead, both = (D3 - 100, D3 + 300, 1), (D3 - 100, E3 + 100, 1)
    wins = [lead, both, (D3, D3 + 300, 1)]
    arms = [("three segments of 300 one-node pieces", (D3, D3 + 300, 1), lambda P, c: P.np == 900 and [len(ch) for ch in P.chains] == [300, 300, 300]),
            ("every node of the tripled stretch is a piece of its own", both, lambda P, c: own_pieces(P, D3, E3, 3)),
            ("a segment of long pieces and one-node pieces, 256 pieces deep", lead, lambda P, c: mixed_segment(P))]
    return Case("strands_3", Unit(4096, cover(1000, 1700) + cover(1150, 1550, OFF + SEP) + cover(1150, 1550, OFF + 2 * SEP)), wins, arms, reprune=(2,))


# ---- branch_lanes ------------------------------------------------------------------------------------------------------------------------

BX = 2048 + 300          # the branch node: BX -> BX + 1 and BX -> BX + 2 (a deletion of one base); BX + 1 is a segment of one node, BX + 2 a head
MULTI = BX + 400         # the single -> multi -> single stretch: a second variant over MULTI + 1 .. MULTI + 149
BHI = MULTI + 300


def branch_windows():
    return [(lo, BHI, 1) for lo in list(range(BX - 258, BX - 252)) + list(range(BX - 130, BX + 1))]


def case_branch_lanes():
    """lo moves the branch node, the one-node segment behind it and the head behind that over every lane of three wavefronts and over the edge of a 256-thread block."""
    ps = cover(BX - 400, MULTI + 1) + [dele(BX, [1])]
    Y = MULTI + 150
    ps += [span(MULTI, MULTI + OFF)] + variants(MULTI + 1, 2, start_at, MULTI + 1 + OFF) + variants(Y, 2, end_at) + [span(Y, Y + OFF)] + cover(Y + 1, Y + 400)

    def w(lo):
        return (lo, BHI, 1)

    def at(off, lane, block_last=False):
        """the node BX + off sits on `lane` (and on the last id of a 256-block)"""
        return lambda P, c: id_at(P, BX + off) % 64 == lane and (not block_last or id_at(P, BX + off) % 256 == 255)
    arms = [("the branch node has two links, BX + 1 is a segment of one node with one link, BX + 2 a head with two predecessors", w(BX - 130),
             lambda P, c: P.outdeg[id_at(P, BX)] == 2 and is_tail(P, id_at(P, BX)) and is_head(P, id_at(P, BX + 1)) and is_tail(P, id_at(P, BX + 1))
             and is_head(P, id_at(P, BX + 2)) and P.indeg[id_at(P, BX + 2)] == 2),
            ("the branch node is a tail at lane 63", w(BX - 63), at(0, 63)), ("the branch node is a tail at lane 0", w(BX), at(0, 0)),
            ("the branch node is a tail at lane 0 of the second wavefront", w(BX - 64), at(0, 0)),
            ("the branch node is the last id of a 256-block", w(BX - 255), at(0, 63, True)),
            ("the branch node is the first id of the second 256-block", w(BX - 256), lambda P, c: id_at(P, BX) == 256),
            ("a head at lane 0 (the one-node segment)", w(BX - 63), at(1, 0)), ("a head at lane 63, a one-node segment at lane 63", w(BX - 62), at(1, 63)),
            ("a head at lane 0 behind a one-node segment at lane 63", w(BX - 62), at(2, 0)), ("a head at lane 63 (where the strands merge)", w(BX - 61), at(2, 63)),
            ("a head on the first id of the second 256-block", w(BX - 254), lambda P, c: id_at(P, BX + 2) == 256),
            ("a piece that ends at lane 63 and whose node links on", w(BX - 130), lambda P, c: P.nxt[63] == 64 and not P.link[63] and P.piece_of[64] == P.piece_of[63] + 1),
            ("the second variant's strand: a head and a tail that are variant 1", w(BX - 130),
             lambda P, c: any(P.var[h] == 1 for h in P.heads) and any(P.var[t] == 1 for t in P.tails))]
    return Case("branch_lanes", Unit(6 * 1024, ps), branch_windows(), arms, reprune=(2,))


# ---- fans --------------------------------------------------------------------------------------------------------------------------------

def _at(i, ln):
    return 2048 + i * 1024 + ln


F4, F5, F9, F4X, FP, FD, F9R = _at(0, 20), _at(1, 20), _at(2, 20), _at(3, 20), _at(5, 20), _at(7, 63), _at(8, 20)


def fans_unit():
    """edge_units' recipes: case_overflow (4, 5 and 9 successors; four spilling sources in a row), case_overflow_pruned, case_overflow_dup; one region each."""
    ps = []
    for x, ds in ((F4, (1, 2, 3)), (F5, (1, 2, 3, 4)), (F9, range(1, 9)), (F9R, range(8, 0, -1))):      # (F9R: the longest deletion first in the file)
        ps += cover(x - 150, x + 200) + [dele(x, [d]) for d in ds]
    ps += cover(F4X - 150, F4X + 200) + [dele(F4X + j, [d]) for j in range(4) for d in range(1, 7)]
    ps += [end_at(FP + 2, FP + 2 + OFF)] * 4 + [end_at(FP - 60, FP - 60 + OFF)] * 4 + [dele(FP, [d]) for d in range(1, 9)]
    ps += cover(FD - 150, FD + 1) + [span(FD, FD + OFF)] + [start_at(FD + 1, FD + 1 + OFF + SEP)] + cover(FD + 1, FD + 200) + [dele(FD, [d]) for d in range(1, 9)]
    return Unit(12 * 1024, ps)


def links_of(P, i):
    return [h for t, h in P.links if t == i]


def on_list(c, x):
    """target positions of the overflow entries of source position x"""
    return {xs for a, xs, _ in c.ovf if a == x}


def case_fans():
    """Tails with 4, 5 and 9 links; the overflow list as the only kept successor (threshold 8 on the overflow_pruned shape: FP's slots hold FP + 1 .. FP + 4, which
    are pruned there, and of the listed targets only FP + 9 has the coverage), as part of a tail's links, cut by the window's end, and listing a pair twice."""
    n = 12 * 1024
    w4, w5, w9, w9cut, w4x = (F4 - 100, F4 + 200, 1), (F5 - 100, F5 + 200, 1), (F9 - 100, F9 + 200, 1), (F9 - 100, F9 + 5, 1), (F4X - 100, F4X + 200, 1)
    wp8, wp4, wp7, wd = (FP - 100, FP + 200, 8), (FP - 100, FP + 200, 4), (FP - 100, FP + 9, 7), (FD - 100, FD + 200, 1)
    w9r = (F9R - 100, F9R + 200, 1)
    wins = [w4, w5, w9, w9cut, w4x, wp8, wp4, wp7, wd, w9r, (0, n, 1), (0, n, 4), (0, n, 8), (FD, FD + 10, 1), (F9, F9 + 10, 1)]

    def tail_links(x, k):
        return lambda P, c: is_tail(P, id_at(P, x)) and len(links_of(P, id_at(P, x))) == k

    def inline_and_list(P, c):
        tgt = {int(P.pos[h]) for h in links_of(P, id_at(P, F9))}
        return len(tgt) == 9 and len(tgt & on_list(c, F9)) >= 1 and len(tgt - on_list(c, F9)) >= 1

    def only_listed(x, t):
        return lambda P, c: P.outdeg[id_at(P, x)] == 1 and P.nxt[id_at(P, x)] == id_at(P, t) >= 0 and t in on_list(c, x) and P.pos[P.nxt[id_at(P, x)]] == t

    def listed_twice(P, c):
        twice = [xs for a, xs, again in c.ovf if a == FD and again]
        tgt = [int(P.pos[h]) for h in links_of(P, id_at(P, FD))]
        return len(twice) >= 1 and all(tgt.count(xs) == 1 for xs in twice if xs > FD + 1) and any(xs > FD + 1 for xs in twice)
    def out_of_order(P, c):
        tgt = {int(P.pos[h]) for h in links_of(P, id_at(P, F9R))}
        return len(tgt) == 9 and len(tgt - on_list(c, F9R)) >= 2 and min(on_list(c, F9R)) < max(tgt - on_list(c, F9R))
    arms = [("a tail with 4 links, none on the list", w4, lambda P, c: tail_links(F4, 4)(P, c) and not on_list(c, F4)),
            ("a tail with 5 links", w5, tail_links(F5, 5)), ("a tail with 9 links", w9, tail_links(F9, 9)),
            ("a tail whose links come from inline slots and from the list", w9, inline_and_list),
            ("a window that cuts between a fan's targets", w9cut, lambda P, c: tail_links(F9, 4)(P, c) and P.hi - 1 == F9 + 4 and len(on_list(c, F9)) >= 5),
            ("four spilling sources in a row", w4x, lambda P, c: all(tail_links(F4X + j, 7)(P, c) and on_list(c, F4X + j) for j in range(4))),
            ("a node whose only kept successor is on the overflow list, the edge internal (threshold)", wp8, only_listed(FP, FP + 9)),
            ("a node whose only kept successor is on the overflow list, the edge internal (threshold and window edge)", wp7, only_listed(FP, FP + 8)),
            ("the overflow_pruned shape: of the slots only FP + 1 is kept, the listed targets are", wp4,
             lambda P, c: sorted(int(P.pos[h]) - FP for h in links_of(P, id_at(P, FP))) == [1, 5, 6, 7, 8, 9] and {FP + d for d in range(5, 10)} <= on_list(c, FP)),
            ("an edge the executor lists twice is one link", wd, listed_twice),
            ("a tail at local id 0 with links from the list", (FD, FD + 10, 1), lambda P, c: id_at(P, FD) == 0 and len(links_of(P, 0)) >= 5),
            ("a tail's links not in insertion order: a listed target lies in front of an inline one", w9r, out_of_order)]
    return Case("fans", fans_unit(), wins, arms, reprune=(4, 8), edges=True, support=True)


# ---- islands -----------------------------------------------------------------------------------------------------------------------------

def case_islands():
    """Strands of 95 kept nodes (a read's arrivals but the last) at 200, 400 and 800 (two overlapping reads) with empty positions between them."""
    ps = [pair(200, 1200), pair(400, 1400), pair(800, 1800), pair(860, 1860)]
    empty = [(300, 400, 1), (0, 200, 1), (295, 296, 1)]
    ends, mid, one, gaps = (294, 401, 1), (250, 300, 1), (200, 201, 1), (190, 300, 1)
    wins = empty + [ends, mid, one, gaps, (0, 4096, 1), (0, 4096, 0), (294, 295, 1)]
    arms = [("a window with no kept node", empty[0], lambda P, c: P.kept == 0), ("a window in front of the first node", empty[1], lambda P, c: P.kept == 0),
            ("a window of one position that holds a pruned node", empty[2], lambda P, c: P.kept == 0 and c.pm((295, 296, 0)).kept == 1),
            ("kept = 1", one, lambda P, c: P.kept == 1 and P.np == 1 and not P.links),
            ("a window whose first and last positions are empty", gaps, lambda P, c: P.kept == 95 and P.pos.min() > P.lo and P.pos.max() < P.hi - 1),
            ("two segments of one node without links", ends, lambda P, c: P.kept == 2 and P.np == 2 and len(P.heads) == 2 and not P.links),
            ("a window that starts in the middle of a strand: the head's predecessor lies in front of lo", mid,
             lambda P, c: P.pos[0] == P.lo and len(P.heads) == 1 and id_at(c.pm((0, 4096, 1)), P.lo) >= 0 and c.pm((0, 4096, 1)).haspred[id_at(c.pm((0, 4096, 1)), P.lo)])]
    return Case("islands", Unit(4096, ps), wins, arms, empty=empty, reprune=(0, 2))


# ---- bases -------------------------------------------------------------------------------------------------------------------------------

TIE = 2048 + 100
NOVOTE = (4096 + 10, 4096 + 1024 + 11, 4096 + 1024 + 512 + 12)


def case_bases():
    """Two reads of one variant that differ at four read indices (votes 1 : 1 for A/C, C/G, G/T, T/N); reads whose last arrival, which votes for nothing, lies on a contig."""
    import walk_units as WU
    ps = [pair(TIE, TIE + OFF, bases={20: "A", 30: "C", 40: "G", 50: "T"}), pair(TIE, TIE + OFF, bases={20: "C", 30: "G", 40: "T", 50: "N"})]
    contigs = []
    for z in NOVOTE:
        ps += [end_at(z, z + OFF)]
        contigs += [(z - 150, z + 150, "+")]
    n = 8 * 1024
    wt, wz, whigh = (TIE - 50, TIE + 150, 1), (NOVOTE[0] - 200, NOVOTE[-1] + 200, 1), (0, n, HIGH)

    def tie(a, b):
        def fn(P, c):
            v = P.cnt[:, 1:6]
            top = np.sort(v, axis=1)
            return bool(((top[:, -1] == top[:, -2]) & (top[:, -1] > 0) & (v[:, a] == top[:, -1]) & (v[:, b] == top[:, -1])).any())
        return fn

    def no_votes(P, c):
        m = (P.cnt[:, 1:6].sum(axis=1) == 0)
        return m.any() and any(c.ref[int(x)] != ord("A") for x in P.pos[m]) and len({c.ref[int(x)] for x in P.pos[m]}) >= 2
    arms = [("a kept node whose two highest votes tie: %s = %s" % ("ACGTN"[a], "ACGTN"[b]), wt, tie(a, b)) for a, b in ((0, 1), (1, 2), (2, 3), (3, 4))]
    arms += [("kept nodes without a vote whose reference bases differ and are not all A", wz, no_votes),
             ("a threshold that leaves only contig nodes", whigh, lambda P, c: 0 < P.kept < c.pm((0, n, 1)).kept and (c.g["node_key"].reshape(-1, 6)[P.node, 0] != NONE).all())]
    return Case("bases", WU.WUnit(n, ps, contigs), [wt, wz, whigh, (0, n, 1), (0, n, 0)], arms, reprune=(HIGH, 0))


# ---- map_edges ---------------------------------------------------------------------------------------------------------------------------

def case_map_edges():
    """The id map on strands_2's unit: the first strand's nodes are main ids (a window's id i is position lo + i), the second strand's are side ids (the window's ids from
    n_main = hi - lo on): both strands are runs of consecutive ids, so a run crosses every 64-id boundary it meets, the main run ends on the last main id where the window
    ends inside the doubled stretch, and the side run starts at n_main."""
    a64, a65, lead = (D2 + 10, D2 + 10 + 128, 1), (D2 + 10, D2 + 10 + 129, 1), (D2 - 100, D2 + 91, 1)
    gap, dead, tail_end = (900, D2 + 60, 1), (D2 - 100, D2 + 400, 3), (E2 - 64, 3700, 1)
    wins = [a64, a65, lead, gap, dead, tail_end, (0, 8192, 1)]
    arms = [("n_main a multiple of 64; the main run ends on the last main id, the side run starts at n_main", a64,
             lambda P, c: (P.hi - P.lo) % 64 == 0 and P.kept == 2 * (P.hi - P.lo) and len(P.heads) == 2),
            ("n_main no multiple of 64; the same", a65, lambda P, c: (P.hi - P.lo) % 64 == 1 and P.kept == 2 * (P.hi - P.lo) and len(P.heads) == 2),
            ("a run of main ids across a 64-id boundary whose nodes are not consecutive local ids", lead,
             lambda P, c: len(P.heads) == 2 and seg_len(P, 0) == P.hi - P.lo > 64 and (np.diff(P.pos[P.seg_of == 0]) == 1).all()),
            ("main ids without a node inside the window", gap, lambda P, c: P.pos.min() > P.lo + 50),
            ("side ids (and main ids) dead at the threshold", dead, lambda P, c: 0 < ((P.var == 1)).sum() < (c.pm((D2 - 100, D2 + 400, 1)).var == 1).sum()),
            ("the side run ends in front of the window's last main ids", tail_end, lambda P, c: P.pos[P.var == 1].max() < P.pos.max() - 100)]
    X, S64, END = "a run of main ids across a 64-id boundary", "a run of side ids across a 64-id boundary", "a run ends on the last main id and a side run starts at n_main"
    want = {a64: {X, S64, END, "n_main is a multiple of 64"}, a65: {X, S64, END, "n_main is no multiple of 64"}, lead: {X, END}, gap: {"a main id without a node in the export", END},
            dead: {"a side id dead at the threshold", "a main id without a node in the export"}, tail_end: {X, "a main id without a node in the export"}}
    return Case("map_edges", strands_unit(), wins, arms, maps=wins, map_want=want)


def cases():
    return [case_straight(), case_strands_2(), case_strands_3(), case_branch_lanes(), case_fans(), case_islands(), case_bases(), case_map_edges()]
