"""Hand-made units that pin the walk preparation (agx_k_assign_aid, agx_k_emit_alive, agx_k_special_bits, agx_k_special_emit, agx_k_fetch_records;
agx_kernels.hip) path by path.

The units are lean_units.Unit's (plus, here, contigs aligned in several PSL blocks), so the CPU twin (tests/test_walk_graph_cases.py) and the GPU file
(tests/test_gpu_walk_graph.py) build exactly the same inputs.  Each case names the paths it is there for as predicates on what the serial executor
reports (hostsim.sim.run(..., graph=True, walk=True)): check_paths() asserts them, so a case cannot silently stop reaching its path.  What is correct
is decided by tests/walk_model.py from the oracle's graph; nothing here works out expected values, except the ids a case of the special rule names.

Coverage: a read's arrival at its LAST aligned position only ever names that node as a successor (AG:1501-1505) and adds no coverage and no vote
there, so a node that only such arrivals reach has coverage 0 and no consensus base: it is pruned unless a contig runs through its position.

Not reachable with the loaders: more chain ends than positions (n_chain_end > n_pos, the other operand of agx_launch_compact's first grid): a chain is
one placement of a contig of more than 200 bases (AG:839), so a unit holds fewer than n_pos / 200 of them.
"""
import os

import numpy as np

import edge_units as EU
import lean_units as LU
from edge_units import OFF, SEP, cover, dele, end_at, span, start_at
from lean_units import K, L, Unit, pair

NONE = 0xFFFFFFFF
CONT, CONTIG, SIDE, ANY, ABSENT = 1, 2, 4, 8, 128
BLOCK = 1024            # positions per block of agx_k_assign_aid / agx_k_emit_alive (256 threads, 4 positions each, 256 apart)
SEG_INDEX = 1024        # positions per entry of the device's index of the rank-0 runs


class WUnit(Unit):
    """gapped: contigs aligned in several blocks, (start, block length, gap, blocks): the contig is the blocks' bases joined, every block aligned
    `gap` positions behind the last one's end: one rank-0 run of conti-mers per block."""

    def __init__(self, genome_len, pairs, contigs=(), gapped=(), seed=11):
        Unit.__init__(self, genome_len, pairs, contigs, seed)
        self.gapped = list(gapped)


def write_unit(unit, run):
    tmp = LU.write_unit(unit, run)
    gapped = getattr(unit, "gapped", ())
    if gapped:
        g = "".join(l.strip() for l in open(os.path.join(tmp, "_genome.0.fa")).read().split("\n")[1:])
        with open(os.path.join(tmp, "_contigs.fa"), "a") as cf, open(os.path.join(tmp, "_contigs_genome.0.psl"), "a") as pf:
            for j, (s, bl, gap, nb) in enumerate(gapped):
                i = len(unit.contigs) + j
                t = [s + b * (bl + gap) for b in range(nb)]
                seq, n, name = "".join(g[x:x + bl] for x in t), nb * bl, "%d.%d" % (i, i)
                cf.write(">%s\n%s\n" % (name, "".join(seq[q:q + 60] + "\n" for q in range(0, n, 60)).rstrip("\n")))
                pf.write("%d\t0\t0\t0\t0\t0\t%d\t%d\t+\t%s\t%d\t0\t%d\t0\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (
                    n, nb - 1, (nb - 1) * gap, name, n, n, unit.genome_len, s, t[-1] + bl, nb, "".join("%d," % bl for _ in t),
                    "".join("%d," % (b * bl) for b in range(nb)), "".join("%d," % x for x in t)))
    return tmp


class Case:
    def __init__(self, name, group, unit, want, coverage=1, iv=LU.IV, jumps=False, small_caps=False, sparse_min=False, special_ids=None):
        """want: [(description, fn(View) -> bool)]; jumps: the case has side ids and jumps (the GPU file also runs it with the upload in three windows and
        the streamed download in 2 and 16 pieces); small_caps / sparse_min: the GPU file also runs it under AGX_TEST_SMALL_CAPS=1 / AGX_FLAG_SPARSE_MIN;
        special_ids: fn(View) -> ids that the case's clause of the special rule makes special (asserted on the executor AND on the model)."""
        self.name, self.group, self.unit, self.want, self.coverage, self.iv = name, group, unit, want, coverage, iv
        self.jumps, self.small_caps, self.sparse_min, self.special_ids = jumps, small_caps, sparse_min, special_ids


class View:
    """What the predicates look at: the executor's walk graph and node table, digested."""

    def __init__(self, out, coverage):
        w, g = out["walk"], out["graph"]
        self.w, self.g, self.coverage = w, g, coverage
        self.n_pos, self.n_ids = int(w["n_pos"]), int(w["n_ids"])
        self.meta = w["meta"].astype(np.int64)
        self.next = w["all_node"]["next"].astype(np.int64)
        self.n_words = self.n_ids // 64 + 1
        self.special = ((w["sp_bits"][:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:self.n_ids]
        self.xpos = np.concatenate((np.arange(self.n_pos), w["side_xpos"].astype(np.int64)))
        self.per_pos = np.diff(g["node_start"].astype(np.int64))
        self.alive_node = (g["node_key"][:, 0] != NONE) | (g["node_cnt"][:, 0] >= coverage)
        pos_of = np.repeat(np.arange(self.n_pos), self.per_pos)
        self.alive_at = np.bincount(pos_of[self.alive_node], minlength=self.n_pos)
        first = np.zeros(self.n_pos, bool)      # the position's first variant is alive
        has = self.per_pos > 0
        first[has] = self.alive_node[g["node_start"].astype(np.int64)[:-1][has]]
        # kinds of positions: E empty, A1 / P1 one variant alive / pruned, VA several with the first alive, VPA first pruned and a later one alive, VPP all pruned
        self.kind = np.where(self.per_pos == 0, "E", np.where(self.per_pos == 1, np.where(first, "A1", "P1"), np.where(first, "VA", np.where(self.alive_at > 0, "VPA", "VPP"))))
        es = g["edge_start"].astype(np.int64)
        self.e_src_pos = pos_of[np.repeat(np.arange(len(pos_of)), np.diff(es))]
        self.e_dst_pos = pos_of[g["edge_dst"].astype(np.int64)]
        self.deg_all = np.diff(es)
        self.node_pos = pos_of
        self.ovf = w["ovf"].astype(np.int64)
        # conti-mers per position and the device's search for a position's rank-0 run (agx_k_special_emit)
        segs = w["segs"]
        self.cm = np.zeros(self.n_pos + 1, np.int64)
        for s in segs:
            a, b = int(s["pos0"]), int(s["pos0"]) + int(s["len"])
            self.cm[a:b] = np.maximum(self.cm[a:b], int(s["rank"]) + 1)
        self.n_seg0 = int(w["n_seg0"])
        self.seg0 = segs[:self.n_seg0]

    def hop_len_of(self):
        """special id -> bases its hop entry appends"""
        return dict(zip(np.nonzero(self.special)[0].tolist(), self.w["sp_hop"]["len"].tolist()))

    def succ(self, a):
        return sorted(set(int(t) for t in self.next[a] if t != NONE) | set(int(d) for s, d in self.ovf if s == a))

    def hop_search(self):
        """per special id whose position holds one conti-mer: (id, position, forward steps from the index entry of its 64-id word, index of the run that holds it or -1)"""
        out = []
        if not self.n_seg0:
            return out
        p0 = self.seg0["pos0"].astype(np.int64)
        sp = np.nonzero(self.special)[0]
        for wd in np.unique(sp // 64):
            ids = sp[sp // 64 == wd]
            s0 = int(self.w["seg_index"][int(self.xpos[ids].min()) // SEG_INDEX])
            for a in ids:
                x = int(self.xpos[a])
                if self.cm[x] != 1:
                    continue
                last = max(int(np.searchsorted(p0, x, "right")) - 1, s0)
                g = self.seg0[last]
                inside = int(g["pos0"]) <= x < int(g["pos0"]) + int(g["len"])
                out.append((int(a), x, last - s0, last if inside else -1))
        return out


def check_paths(case, out):
    v = View(out, case.coverage)
    for what, fn in case.want:
        assert fn(v), "%s: %s" % (case.name, what)
    return v


# ---- thread layout -----------------------------------------------------------------------------------------------------------------------

def _seg(kind, reads):
    return reads * 2 if kind == "A" else reads if kind == "P" else []


def _layout_pairs(G):
    """Alive (A: two reads, coverage 2), pruned (P: one) and empty (E) stretches on either side of every multiple of 256 below G, a forced run across
    every odd multiple of 1024, and a run onto the unit's last position (alive by the contig case_layout lays there)."""
    combos = [("A", "P"), ("P", "A"), ("A", "E"), ("E", "A"), ("P", "E"), ("E", "P"), ("P", "P"), ("A", "A")]
    ps, last = [], G - 1
    for k, b in enumerate(range(256, G, 256)):
        if b + 100 > G - 100 and b + 100 > G:      # no room for a read that starts here: the run that ends on the last position crosses it
            continue
        if b % BLOCK == 0 and (b // BLOCK) % 2 == 1:
            ps += [pair(b - 50, b - 50)] * 2
            continue
        kl, kr = combos[k % len(combos)]
        ps += _seg(kl, [pair(b - 97, b - 97, "97M3S", "97M3S")]) + _seg(kr, [pair(b, b)])      # (97M3S: the stretch's last node, without coverage of its own, is b - 1)
    ps += [pair(last - 96, last - 96, "97M3S", "97M3S")] * 2 + [pair(last - 95, last - 95, "96M4S", "96M4S")] * 2
    if G < 512:
        ps += [pair(0, 0, "60M40S", "60M40S")]      # a pruned stretch in front of the contig
    return ps


def _end_contig(G, n=210):
    """A contig over the unit's last n positions: the node at the last position has no coverage of its own (module comment) and lives by the contig."""
    return [(G - n, G, "+")]


def _crosses(v, b):
    return b < v.n_pos and bool(v.meta[b - 1] & CONT) and bool(v.meta[b] & CONT)


def case_layout(G):
    """Thread layout of agx_k_assign_aid / agx_k_emit_alive (X = block * 1024 + thread + 256 * j) at n_pos = G, coverage 2."""
    want = [("n_pos", lambda v: v.n_pos == G),
            ("a node at the unit's last position, reached from the one before", lambda v: v.per_pos[G - 1] >= 1 and (G - 1) in v.succ(G - 2))]
    bs = [b for b in range(256, G, 256) if b + 100 <= G]
    if len(bs) >= 3:
        want += [("different kinds of neighbours across the 256-boundaries", lambda v: len({(v.kind[b - 1], v.kind[b]) for b in bs}) >= min(len(bs), 4))]
    if any(b % BLOCK == 0 and (b // BLOCK) % 2 == 1 for b in bs):
        want += [("a forced run across a block boundary", lambda v: any(_crosses(v, b) for b in bs if b % BLOCK == 0))]
    if G >= 4096:
        want += [("alive, pruned and empty positions next to boundaries", lambda v: {"A1", "P1", "E"} <= {v.kind[x] for b in bs for x in (b - 1, b)})]
    if G < 512:
        want += [("a pruned stretch", lambda v: "P1" in set(v.kind.tolist()))]
    return Case("layout_%d" % G, "layout", Unit(G, _layout_pairs(G), _end_contig(G)), want, coverage=2)


def case_layout_min():
    """The smallest unit that holds a pair of reads of 100 bases whose left mate is the one further left: 101 positions."""
    return Case("layout_min", "layout", Unit(101, [pair(0, 1)] * 2), [("n_pos", lambda v: v.n_pos == 101), ("a node at position 0", lambda v: v.kind[0] == "A1")], coverage=2)


def case_last_side():
    """The last main ids with successors in the side block: two variants at the unit's last position (insertVariation 0, as edge_units.case_unit_end), the
    position before it steps to both.  (The last main id itself can have no successor: every step goes to a later position.)"""
    G = 64 * 70 + 37      # (above 4 096 positions: the unit's download can be streamed)
    last = G - 1
    ps = cover(1000, 1400) + cover(last - 300, last - 100, 0)
    ps += [pair(last - 95, last - 95, "96M4S", "96M4S"), pair(last - 96, last - 96, "97M3S", "97M3S"), pair(last - 95, last - 95, "96M4S", "69M26I5M")]
    # (the other mate's insertion of 26 bases puts its position at index 95 26 behind the first read's: a variant of its own at insertVariation 0, whose contig offset is
    # still within 25 of the stored one at the position before, so the step is allowed, AG:1589-1623)
    want = [("two variants at the last position", lambda v: v.per_pos[v.n_pos - 1] == 2 and v.n_ids == v.n_pos + 1),
            ("main id n_pos - 2 steps to the side id n_pos", lambda v: v.n_pos in v.succ(v.n_pos - 2)),
            ("the mixed word holds the last main ids and the side id", lambda v: v.n_pos % 64 != 0)]
    return Case("last_side", "layout", Unit(G, ps, _end_contig(G, 300)), want, iv=0, jumps=True, special_ids=lambda v: [v.n_pos - 2, v.n_pos - 1, v.n_pos])


# ---- one-variant fast path against the general path ----------------------------------------------------------------------------------------

def _at(i, ln, gap=1024, first=2048):
    return first + i * gap + ln


def case_kinds():
    """Neighbouring positions with no variant, one alive, one pruned, several with the first alive, the first pruned and a later one alive, and all
    pruned, at coverage 2: the kinds as sources and targets of each other; single successors that are id + 1, a side id, an id further on (a
    deletion's jump) and a pruned node; a one-variant node with four slot entries of which two are pruned; nodes without a consensus base (reached
    only as successors, on a contig) alone at a position and beside another variant."""
    ps, contigs = [], []
    A, P = 2, 1

    def run(x, n, m_off=OFF, first=None):
        """n reads whose first arrival is x"""
        return [start_at(x, x + m_off)] * n

    # 0: A1 -> P1 -> E: an alive stretch, one read goes on alone
    x = _at(0, 10); ps += run(x, A) + [start_at(x + 50, x + 50 + OFF)]
    # 1: P1 -> A1: a lone read runs into an alive stretch
    x = _at(1, 10); ps += [start_at(x, x + OFF)] + run(x + 60, A)
    # 2: A1 -> VA -> A1: over part of an alive stretch other reads (mates SEP further, first in the file: their variant comes first) hold the main ids; the stretch's own
    # nodes are side ids there: a main id whose single successor is a side id
    x = _at(2, 10); ps += [start_at(x + 30, x + 30 + OFF + SEP)] * A + run(x, A) + run(x + 96, A)
    # 3: A1 -> VPA: the first variant of a stretch is a lone read's (pruned), the alive reads' mates lie SEP further and arrive later
    x = _at(3, 10); ps += [start_at(x + 40, x + 40 + OFF)] + [start_at(x, x + OFF + SEP)] * A + [start_at(x + 90, x + 90 + OFF + SEP)] * A
    # 4: P1 -> VPP -> P1: two lone reads with mates SEP apart
    x = _at(4, 10); ps += [start_at(x, x + OFF)] + [start_at(x + 40, x + 40 + OFF + SEP)]
    # 11, 12: VPP and VPA stretches with empty positions on both sides
    x = _at(11, 10); ps += [start_at(x, x + OFF), start_at(x, x + OFF + SEP)]
    x = _at(12, 10); ps += [start_at(x, x + OFF)] + [start_at(x, x + OFF + SEP)] * A
    # 5: VA -> VPA and VPA -> VA: which variant comes first changes along a stretch (the first variant's reads end, a lone read with their mates goes on)
    x = _at(5, 10); ps += [start_at(x, x + OFF)] * A + [start_at(x + 20, x + 20 + OFF + SEP)] * A + [start_at(x + 60, x + 60 + OFF)] + [start_at(x + 110, x + 110 + OFF + SEP)] * A
    # 6: a jump: the only alive successor lies further on (the reads that step to x + 1 are too few)
    x = _at(6, 10); ps += [end_at(x + 1, x + 1 + OFF)] * A + [dele(x, [6])] * A
    # 7: four slot entries, one of them pruned: x + 1 alive, x + 2 reached by one read (pruned), x + 3 and x + 4 by that one and the later ones (alive)
    x = _at(7, 10); ps += [end_at(x + 2, x + 2 + OFF)] * A + [dele(x, [1]), dele(x, [2]), dele(x, [3])]
    # 8: a single successor that is pruned: an alive stretch whose reads end, one read goes on
    x = _at(8, 10); ps += [end_at(x + 1, x + 1 + OFF)] * A + [span(x, x + OFF, q=5)]
    # 9, 10: no consensus base: the last node of a read on a contig, alone (fast path) and with a second variant (general path)
    x = _at(9, 10); ps += [end_at(x, x + OFF)]; contigs += [(x - 150, x + 150, "+")]
    x = _at(10, 10); ps += [end_at(x, x + OFF), end_at(x, x + OFF + SEP)]; contigs += [(x - 150, x + 150, "+")]

    def pairs_of(v):
        return {(v.kind[a], v.kind[b]) for a, b in zip(v.e_src_pos, v.e_dst_pos)}

    def one_alive(v):
        return [int(x) for x in np.nonzero(v.kind == "A1")[0]]

    def no_votes(v, several):
        n = v.g["node_cnt"]
        return any(v.alive_node[i] and not n[i, 1:].any() and (v.per_pos[v.node_pos[i]] > 1) == several for i in range(len(n)))

    kinds = ["A1", "P1", "VA", "VPA", "VPP"]
    want = [("every kind of position occurs", lambda v: set(kinds) | {"E"} <= set(v.kind.tolist()))]
    want += [("%s is the source of a step to another kind" % k, lambda v, k=k: any(a == k and b != k for a, b in pairs_of(v))) for k in kinds]
    want += [("%s is the target of a step from another kind" % k, lambda v, k=k: any(b == k and a != k for a, b in pairs_of(v))) for k in kinds]
    want += [("%s next to an empty position" % k, lambda v, k=k: any(v.kind[x] == k and (v.kind[x + 1] == "E" or v.kind[x - 1] == "E") for x in range(1, v.n_pos - 1))) for k in kinds]
    want += [("one variant, single successor id + 1", lambda v: any(v.meta[x] & CONT for x in one_alive(v))),
             ("one variant, single successor a side id", lambda v: any(len(v.succ(x)) == 1 and v.succ(x)[0] >= v.n_pos for x in one_alive(v))),
             ("one variant, single successor further on", lambda v: any(len(v.succ(x)) == 1 and v.n_pos > v.succ(x)[0] > x + 1 for x in one_alive(v))),
             ("one variant, every successor pruned", lambda v: any(v.deg_all[v.g["node_start"][x]] >= 1 and not v.succ(x) for x in one_alive(v))),
             ("one variant, four slot entries, some pruned", lambda v: any(v.deg_all[v.g["node_start"][x]] == 4 and 1 <= len(v.succ(x)) < 4 for x in one_alive(v))),
             ("no consensus base, one variant", lambda v: no_votes(v, False)), ("no consensus base, several variants", lambda v: no_votes(v, True))]
    return Case("kinds", "kinds", Unit(16 * 1024, ps, contigs), want, coverage=2, jumps=True, small_caps=True, sparse_min=True)


# ---- overflow ----------------------------------------------------------------------------------------------------------------------------

def case_ovf_pruned():
    """At coverage 6.  Source a: x + 1 and the deletion targets 1..4, which are pruned (target d is reached by the d reads of deletions up to d): the
    node spilled, its one alive successor is id + 1, and it must not be CONT; its overflow entry names a pruned target.  Source b: five deletion
    targets and nothing else: the spilled source itself is pruned (coverage 5)."""
    a, b = _at(0, 20), _at(2, 20)
    ps = [end_at(a + 2, a + 2 + OFF)] * 6 + [end_at(a - 60, a - 60 + OFF)] * 6 + [dele(a, [d]) for d in range(1, 5)]
    ps += [dele(b, [d]) for d in range(1, 6)]

    def src(v, x):
        return int(v.g["node_start"][x])
    want = [("source a spilled and keeps id + 1 alone", lambda v: v.deg_all[src(v, a)] == 5 and v.succ(a) == [a + 1] and v.kind[a] == "A1"),
            ("source b spilled and is pruned", lambda v: v.deg_all[src(v, b)] == 5 and v.kind[b] == "P1"),
            ("overflow entries of a pruned source and of a pruned target, all NONE/NONE", lambda v: len(v.ovf) >= 2 and (v.ovf == NONE).all())]
    return Case("ovf_pruned", "overflow", Unit(6 * 1024, ps), want, coverage=6, special_ids=lambda v: [a, a + 1])


def case_ovf_marks():
    """The overflow cases of edge_units at coverage 1: overflow targets are alive, marked, and so special together with the id in front of each."""
    c = EU.case_overflow()
    want = [("alive overflow entries", lambda v: (v.ovf[:, 0] != NONE).sum() >= 5)]
    return Case("ovf_marks", "overflow", c.unit, want, jumps=True, small_caps=True,
                special_ids=lambda v: sorted({int(t) for s, t in v.ovf if s != NONE} | {int(t) - 1 for s, t in v.ovf if s != NONE and not (v.meta[int(t) - 1] & ABSENT)}))


def case_ovf_grid():
    """More overflow entries than positions rounded up to 1024: 100 sources on 4 096 positions (the smallest unit whose download can be streamed), each with
    deletions of 1..62 bases besides x + 1.  The
    grid of agx_k_emit_alive is sized by the overflow capacity then, and its threads beyond n_pos still rewrite overflow entries."""
    G = 4096
    ps = cover(40, 3640, 300)
    for x in range(100, 3600, 35):
        ps += [dele(x, [d], x + 300) for d in range(1, 63)]
    want = [("more overflow entries than positions", lambda v: len(v.ovf) > G and v.n_pos == G),
            ("alive entries beyond index n_pos", lambda v: (v.ovf[G:, 0] != NONE).any())]
    return Case("ovf_grid", "overflow", Unit(G, ps), want, small_caps=True)


# ---- the special rule, clause by clause ------------------------------------------------------------------------------------------------------

def case_special():
    """Coverage 1.  a: a deletion lands in the middle of a forced run (the target and the id before it are special).  b: a deletion lands on the first id
    of a 64-id word (the id before is lane 63 of the word before).  c: a node at position 0.  The unit is 70 words and a bit long: groups of four words
    with one non-empty word, empty groups, and a last group of fewer than four words."""
    G = 64 * 70 + 9
    a, b = 1024 + 20, 2048 + 24
    ps = cover(a - 150, a + 200) + [dele(a, [6])] + cover(b - 150, b + 200) + [dele(b, [39])] + [pair(0, 300)]
    last = G - 1
    ps += [pair(last - 95, last - 95, "96M4S", "96M4S")] * 2

    def groups(v):
        wd = np.zeros((v.n_words + 3) // 4 * 4, bool)
        wd[:v.n_words] = v.w["sp_bits"] != 0
        return wd.reshape(-1, 4).sum(axis=1)
    want = [("the jump's target is inside a forced run", lambda v: v.succ(a) == [a + 1, a + 7] and bool(v.meta[a + 6] & CONT) and bool(v.meta[a + 7] & CONT)),
            ("a target on a word boundary", lambda v: (b + 40) % 64 == 0 and b + 40 in v.succ(b)),
            ("a node at position 0", lambda v: v.kind[0] == "A1"),
            ("the last id is a main id with a node", lambda v: v.n_ids == v.n_pos and v.kind[v.n_pos - 1] != "E"),
            ("groups of four words: one non-empty, all empty; a last group of fewer than four", lambda v: 1 in groups(v) and 0 in groups(v) and v.n_words % 4 != 0)]
    return Case("special", "special", Unit(G, ps, _end_contig(G)), want, special_ids=lambda v: [0, a, a + 1, a + 6, a + 7, b + 39, b + 40, v.n_ids - 1])


# ---- hop entries -----------------------------------------------------------------------------------------------------------------------------

def case_hops():
    """Conti-mers: a contig in 40 blocks of 20 bases, 2 positions apart (40 rank-0 runs inside two index entries: the search takes up to 16 forward steps,
    then bisects), two overlapping contigs (positions with two conti-mers, runs of rank 1), plain contigs, one that ends on the unit's last positions; reads
    with two variants over the runs 12..19 of the gapped contig (side ids: their word's search starts at the index entry of their lowest position), over the
    overlap, in front of the first run, between and behind the contigs; the unit's length is no multiple of 64, so one word holds the last main ids — on a
    contig — and the first side ids, which lie 17 runs and more in front."""
    G = 64 * 160 + 21
    s0 = 3 * 1024 + 4
    gapped = [(s0, 20, 2, 40)]
    contigs = [(1024 + 100, 1024 + 500, "+"), (5 * 1024, 5 * 1024 + 400, "+"), (5 * 1024 + 300, 5 * 1024 + 700, "-"), (7 * 1024, 7 * 1024 + 300, "-"),
               (8 * 1024 + 10, 8 * 1024 + 260, "+"), (G - 320, G - 2, "+")]
    ps = []

    def two(x, off=OFF):
        return [end_at(x, x + off), end_at(x, x + off + SEP)]
    ps += two(200)                                           # in front of the first run
    ps += two(1024 + 100 + 40) + two(1024 + 500 + 45)        # across a run's first base; across its last base and behind it
    for x in (s0 + 12 * 22 + 95, s0 + 16 * 22 + 95):         # runs 12 .. 20 of the gapped contig, gaps included
        ps += two(x)
    ps += two(5 * 1024 + 350) + two(5 * 1024 + 660)          # two conti-mers; rank-1 run ends, rank-0 chain's end
    ps += two(7 * 1024 + 299 + 40)                           # a chain's last conti-mer and the positions behind it
    ps += two(6 * 1024 + 500)                                # between contigs
    ps += two(9 * 1024 + 500, 250)                                # beyond all but the last run
    ps += [pair(G - 1 - 95, G - 1 - 95, "96M4S", "96M4S")] * 2      # the last main ids, on the last contig

    def steps(v):
        return {s for _, _, s, _ in v.hop_search()}

    def spx(v):
        return {int(x) for x in v.xpos[v.special]}

    def mixed_word(v):
        wd = v.n_pos // 64
        return [h for h in v.hop_search() if h[0] // 64 == wd and h[0] < v.n_pos]
    want = [("positions with 0, 1 and 2 conti-mers under special ids", lambda v: {0, 1, 2} <= {int(v.cm[v.xpos[a]]) for a in np.nonzero(v.special)[0]}),
            ("exactly 15, 16 and 17 rank-0 runs between the index entry and the position, and many more", lambda v: {15, 16, 17} <= steps(v) and max(steps(v)) > 32),
            ("a position in front of the first run", lambda v: min(spx(v)) < int(v.seg0["pos0"][0])),
            ("a position in a gap between two runs, just behind a run's last base and one further", lambda v: {1, 2} <= {x - q for x in spx(v) for q in (x - 1, x - 2) if s0 < x < s0 + 39 * 22 and v.cm[x] == 0 and v.cm[q] == 1 and v.cm[q + 1] == 0}),
            ("a run's first and last base", lambda v: any(r >= 0 and x == int(v.seg0["pos0"][r]) for _, x, _, r in v.hop_search()) and
             any(r >= 0 and x == int(v.seg0["pos0"][r]) + int(v.seg0["len"][r]) - 1 for _, x, _, r in v.hop_search())),
            ("jj == hop_len0 - 1 and hop_len0", lambda v: {0, 1} <= {int(v.seg0["hop_len0"][r]) - (x - int(v.seg0["pos0"][r])) for _, x, _, r in v.hop_search() if r >= 0}),
            ("runs of rank above 0", lambda v: len(v.w["segs"]) > v.n_seg0),
            ("the one conti-mer with a next: a hop that appends bases", lambda v: any(v.cm[v.xpos[a]] == 1 and n > 0 for a, n in v.hop_len_of().items())),
            ("the one conti-mer without a next (a chain's last): an empty hop", lambda v: any(x in set(v.w["chain_end"].tolist()) and v.hop_len_of()[a] == 0 for a, x, _, _ in v.hop_search())),
            ("positions beyond all runs but the last", lambda v: any(x > 9 * 1024 and v.cm[x] == 0 and x > int(v.seg0["pos0"][-2]) + int(v.seg0["len"][-2]) for x in spx(v))),
            ("the mixed word: main ids on one conti-mer that search from a side id's position 17 runs and more in front",
             lambda v: v.n_pos % 64 != 0 and v.n_ids > v.n_pos and any(s >= 17 for _, _, s, _ in mixed_word(v))),
            ("positions behind a contig's last base that hold no conti-mer", lambda v: any(v.cm[x] == 0 and v.cm[x - 1] >= 1 for x in spx(v) if x > 4 * 1024))]
    return Case("hops", "hops", WUnit(G, ps, contigs, gapped), want, jumps=True, small_caps=True, sparse_min=True)


def case_no_contigs():
    """A unit without contigs (n_seg0 == 0): every hop entry is empty."""
    c = EU.case_sweep_slow()
    return Case("no_contigs", "hops", c.unit, [("no runs", lambda v: v.n_seg0 == 0 and len(v.w["segs"]) == 0), ("side ids", lambda v: v.n_ids > v.n_pos)], jumps=True)


def cases():
    return [case_layout(G) for G in (255, 256, 257, 1023, 1024, 1025, 5000)] + [case_layout_min(), case_last_side(), case_kinds(),
            case_ovf_pruned(), case_ovf_marks(), case_ovf_grid(), case_special(), case_hops(), case_no_contigs()]


# every path the cases are there for, by group: tests/test_walk_graph_cases.py checks that no group has lost its cases
GROUPS = ("layout", "kinds", "overflow", "special", "hops")
