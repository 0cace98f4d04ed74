"""Hand-made units that sit ON the edges of the compatibility windows (AG:1293-1312 and the edge test AG:1602-1615), clause by clause.

The predicate has three clauses: A — same contig at the position and contig offsets within 25; B — the same test on the mate position's conti-mer
with the window W = 2 * insertVariation + 25; C — mate positions within W.  The project states it in agx_compatible, the straight-line case of
agx_node_sweep_lane, the device's own arithmetic in agx_sweep_tile_lean, the fused edge write of agx_node_write_lane, agx_edge_allowed, agx_resolve and
agx_key_compatible (agx_core.h, agx_kernels.hip).  The other unit files keep their values well inside or well outside a window; the units here put the
differences at win - 1, win, win + 1 and at the same three on the other side (the unsigned forms have two ends).

The units are lean_units.Unit's with a list of contigs whose PSL lines may have several blocks, a contig-side gap, and several placements (`psl`);
write_unit() writes them, so the CPU twin (tests/test_window_cases.py) and the GPU file (tests/test_gpu_window_cases.py) build exactly the same inputs.
Each case carries `want` predicates fn(o, s) on the ORACLE's graph (o = harness.run_oracle(..., graph=True)) and the serial executor's report
(s = hostsim.sim.run(..., graph=True, edges=True, records=True)): the keys in question differ by exactly the stated amount and do (or do not) share a
node or an edge, and the executor's records, slow list and counters say which path took the arrival or the step.  Nothing here works out expected
values from the code under test, and a case that stops reaching its edge fails its own assertion.

What a read does (lean_units): pair(left, other) emits, at every index q < L - K, an arrival at position left + q whose mate position is other + q; the
arrival at index L - K only names the next position.  Reads of one group share `left`, so their arrivals come in file order at every position and their
mate positions differ by the same amount everywhere: variant 0 is the first read's key and is never widened.
"""
import os
import random

import numpy as np

import edge_units as EU
import lean_units as LU
from lean_units import L, TILE, Unit, pair

IV = LU.IV
NONE = 0xFFFFFFFF
EP25 = 25                 # clause A's window (AG:39, 1296)
OFF, SEP = EU.OFF, EU.SEP
GENERAL_CIGAR = "30M2I20M3D48M"      # three pieces: no lean record fits it (lean_units.case_general)


def window(iv):
    return 2 * iv + 25


class WinUnit(Unit):
    """psl: contigs written behind Unit.contigs, each {"n": length, "strand": "+" / "-", "placements": [[(q, t, len), ..], ..]}: a PSL line per placement
    whose blocks align contig indices q .. q + len (in the strand's orientation) to positions t .. t + len.  The contig's bases are the genome's under
    the first placement's blocks and random elsewhere."""

    def __init__(self, genome_len, pairs, contigs=(), psl=(), seed=11):
        Unit.__init__(self, genome_len, pairs, contigs, seed)
        self.psl = list(psl)


def contig(n, blocks, strand="+", more=()):
    return {"n": n, "strand": strand, "placements": [list(blocks)] + [list(b) for b in more]}


def plain(s, e, strand="+"):
    return contig(e - s, [(0, s, e - s)], strand)


def write_unit(unit, run):
    tmp = LU.write_unit(unit, run)
    if not getattr(unit, "psl", ()):
        return tmp
    rnd = random.Random(unit.seed + 1000)
    g = "".join(l.strip() for l in open(os.path.join(tmp, "_genome.0.fa")).read().split("\n")[1:])
    with open(os.path.join(tmp, "_contigs.fa"), "a") as cf, open(os.path.join(tmp, "_contigs_genome.0.psl"), "a") as pf:
        for j, c in enumerate(unit.psl):
            i, n = len(unit.contigs) + j, c["n"]
            name = "%d.%d" % (i, i)
            seq = [rnd.choice("ACGT") for _ in range(n)]
            for q, t, ln in c["placements"][0]:
                seq[q:q + ln] = g[t:t + ln]
            seq = "".join(seq)
            if c["strand"] == "-":
                seq = LU.revcomp(seq)
            cf.write(">%s\n%s\n" % (name, "".join(seq[q:q + 60] + "\n" for q in range(0, n, 60)).rstrip("\n")))
            for blocks in c["placements"]:
                q0, q1 = blocks[0][0], blocks[-1][0] + blocks[-1][2]
                t0, t1 = blocks[0][1], blocks[-1][1] + blocks[-1][2]
                m = sum(b[2] for b in blocks)
                assert q1 <= n and t1 <= unit.genome_len and all(a[0] + a[2] <= b[0] and a[1] + a[2] <= b[1] for a, b in zip(blocks, blocks[1:]))
                pf.write("%d\t0\t0\t0\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t0\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (
                    m, len(blocks) - 1, q1 - q0 - m, len(blocks) - 1, t1 - t0 - m, c["strand"], name, n, q0, q1, unit.genome_len, t0, t1, len(blocks),
                    "".join("%d," % b[2] for b in blocks), "".join("%d," % b[0] for b in blocks), "".join("%d," % b[1] for b in blocks)))
    return tmp


class Case:
    def __init__(self, name, group, unit, want, coverage=1, iv=IV, reprune=()):
        """want: [(description, fn(o, s) -> bool)]; reprune: the coverages the GPU file re-prunes the built unit to (the reference's answers are recorded
        at `coverage` and at each of them)."""
        self.name, self.group, self.unit, self.want, self.coverage, self.iv, self.reprune = name, group, unit, want, coverage, iv, tuple(reprune)

    def write(self, run):
        return write_unit(self.unit, run)


def check(case, o, s):
    for what, fn in case.want:
        assert fn(o, s), "%s: %s" % (case.name, what)


# ---- the numpy model over the oracle's tables --------------------------------------------------------------------------------------------------------
# node_key columns: contig id, contig offset, mate contig id, mate contig offset, mate chromosome, mate position

def ids_at(o, x):
    ns = o["graph"]["node_start"]
    return list(range(int(ns[x]), int(ns[x + 1])))


def keys_at(o, x, col):
    return [int(o["graph"]["node_key"][i, col]) for i in ids_at(o, x)]


def cov_at(o, x):
    return [int(o["graph"]["node_cnt"][i, 0]) for i in ids_at(o, x)]


def succ(o, i):
    g = o["graph"]
    return set(int(d) for d in g["edge_dst"][int(g["edge_start"][i]):int(g["edge_start"][i + 1])])


def edge(o, x, v, y, w):
    """variant v of position x -> variant w of position y"""
    return ids_at(o, y)[w] in succ(o, ids_at(o, x)[v])


def tile_max(o, x):
    ns = o["graph"]["node_start"].astype(np.int64)
    lo, hi = x // TILE * TILE, min((x // TILE + 1) * TILE, int(o["graph"]["n_pos"]))
    return int((ns[lo + 1:hi + 1] - ns[lo:hi]).max())


def tiles_beyond(o, v):
    """How many tiles hold a position with more than v variants: with v = AGX_MAXV_LDS = 2 the tiles pass 0 of the device's node sweep hands to pass 1 (n_mid_tiles), with
    v = AGX_MAXV_MID = 4 those pass 1 hands to pass 2 (n_big_tiles) — no list here is long enough to leave pass 0 for its length."""
    per = np.diff(o["graph"]["node_start"].astype(np.int64))
    per = np.concatenate([per, np.zeros(-len(per) % TILE, np.int64)]).reshape(-1, TILE)
    return int((per.max(axis=1) > v).sum())


def mates_are(x, want, what):
    """the variants at x, in order: (mate position, coverage)"""
    return ("%s: position %d holds the variants (mate position, coverage) %s" % (what, x, want),
            lambda o, s: list(zip(keys_at(o, x, 5), cov_at(o, x))) == want)


def record_kind(x, kind, rev, what):
    """a lean record of `kind` on strand `rev` in x's tile (the executor's records): the path the tile's arrivals take on the device"""
    return ("%s: a lean record of kind %d%s in tile %d" % (what, kind, " (reverse)" if rev else "", x // TILE),
            lambda o, s: LU.count(s["records"], tile=x // TILE, kind=kind, rev=rev) >= 1)


def no_general(x, what):
    return ("%s: no general record in tile %d" % (what, x // TILE), lambda o, s: LU.count(s["records"], tile=x // TILE, kind=LU.KIND_GENERAL) == 0)


def tile_variants(x, lo, hi, what):
    return ("%s: the most variants at a position of tile %d is in [%d, %d]" % (what, x // TILE, lo, hi), lambda o, s: lo <= tile_max(o, x) <= hi)


KEY_NAMES = ("contig", "contig offset", "mate contig", "mate contig offset", "mate chromosome", "mate position")


def graph_diff(name, go, gd):
    """The first difference between the oracle's tables and another's (the executor's, the device's), in words; None if there is none."""
    if int(go["n_pos"]) != int(gd["n_pos"]):
        return "%s: n_pos %d, the other has %d" % (name, go["n_pos"], gd["n_pos"])
    so, sd = go["node_start"].astype(np.int64), gd["node_start"].astype(np.int64)
    bad = np.nonzero(np.diff(so) != np.diff(sd))[0]
    if len(bad):
        x = int(bad[0])
        return "%s: position %d holds %d variants, the other has %d; keys %s / %s" % (
            name, x, so[x + 1] - so[x], sd[x + 1] - sd[x], go["node_key"][so[x]:so[x + 1]].tolist(), gd["node_key"][sd[x]:sd[x + 1]].tolist())
    pos = np.repeat(np.arange(int(go["n_pos"])), np.diff(so))
    for field, names in (("node_key", KEY_NAMES), ("node_cnt", ("coverage", "A", "C", "G", "T", "N")), ("node_slen", None)):
        a, b = go[field], gd[field]
        rows = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        if len(rows):
            i = int(rows[0])
            x = int(pos[i])
            col = names[int(np.nonzero(np.atleast_1d(a[i] != b[i]))[0][0])] if names else field
            return "%s: position %d variant %d differs in %s (%s): the oracle's key %s count %s, the other's key %s count %s" % (
                name, x, i - so[x], field, col, go["node_key"][i].tolist(), go["node_cnt"][i].tolist(), gd["node_key"][i].tolist(), gd["node_cnt"][i].tolist())
    eo, ed = go["edge_start"].astype(np.int64), gd["edge_start"].astype(np.int64)
    for i in range(int(go["n_nodes"])):
        a, b = sorted(go["edge_dst"][eo[i]:eo[i + 1]].tolist()), sorted(gd["edge_dst"][ed[i]:ed[i + 1]].tolist())
        if a != b:
            x = int(pos[i])
            return "%s: position %d variant %d (key %s): successors %s, the other has %s (as position:variant)" % (
                name, x, i - so[x], go["node_key"][i].tolist(), ["%d:%d" % (pos[d], d - so[pos[d]]) for d in a], ["%d:%d" % (pos[d], d - so[pos[d]]) for d in b])
    return None


# ---- clause C: mate positions ---------------------------------------------------------------------------------------------------------------------------

Q = 10      # the read index whose position the clause-C cases look at


def _group(x, mates, rev, cigar="%dM" % L):
    return [pair(x, m, left_cigar=cigar, rev=rev) for m in mates]


def _c_groups(W, first=1024, gap=512, m_first=10240, cigar="%dM" % L, kinds=(LU.KIND_ONE,), probe=True):
    """The clause-C groups in regions `gap` apart, forward and reverse: the edges on the high side, on the low side, and both orders of arrival.  With probe, a
    contig ends five positions into every group, so that the walk extends it through the group's variants (the output files then depend on them)."""
    ps, want, psl, i = [], [], [], 0
    for rev in (False, True):
        for name, offs, expect in (
                ("high side", (0, W, -W, W + 1), [(0, 3), (W + 1, 1)]),
                ("low side", (0, -W, W, -(W + 1)), [(0, 3), (-(W + 1), 1)]),
                ("inside by one", (0, W - 1, -(W - 1)), [(0, 3)]),
                ("M, M + W, M + 2W", (0, W, 2 * W), [(0, 2), (2 * W, 1)]),
                ("M + 2W, M + W, M", (2 * W, W, 0), [(2 * W, 2), (0, 1)])):
            x, M = first + i * gap + 8, m_first + i * 400 + 2 * W + 10
            i += 1
            ps += _group(x, [M + d for d in offs], rev, cigar)
            what = "%s%s" % (name, ", reverse" if rev else "")
            want.append(mates_are(x + Q, [(M + Q + d, c) for d, c in expect], what))
            want += [record_kind(x + Q, k, rev, what) for k in kinds]
            if LU.KIND_GENERAL not in kinds:
                want += [no_general(x + Q, what), tile_variants(x + Q, 2 if len(expect) > 1 else 1, 2, what + " (pass 0 keeps the tile)")]
            if probe:
                psl.append(plain(x - 220, x + 5))
    return ps, want, psl, first + i * gap


def case_c_lean(iv=IV):
    """C in pass 0's straight-line case: kind ONE records, variant 0 stored by the first arrival's arm, mates at M, M +- W (join variant 0), M +- (W + 1) (a variant of
    their own), M +- (W - 1); M, M + W, M + 2W in both file orders (variant 0 is the first arrival's key and is never widened)."""
    W = window(iv)
    ps, want, psl, end = _c_groups(W)
    want.append(("pass 0 keeps every tile", lambda o, s: tiles_beyond(o, 2) == 0))
    return Case("c_lean" if iv == IV else "c_lean_iv%d" % iv, "C", WinUnit(16 * 1024, ps, psl=psl), want, iv=iv, reprune=(2, 4) if iv == IV else ())


def case_c_general():
    """C behind general records: the same groups with left mates of three pieces (insertion next to a deletion): the device decodes them the general way, their CHAIN
    and jump lanes leave the straight-line case inside a lean tile."""
    ps, want, psl, end = _c_groups(window(IV), cigar=GENERAL_CIGAR, kinds=(LU.KIND_GENERAL,))
    return Case("c_general", "C", WinUnit(16 * 1024, ps, psl=psl), want)


def case_c_mid():
    """C in a tile that pass 1 takes: M, M + W, M - W, M + W + 1, M - (W + 1) at one position make three variants, so the tile leaves pass 0 and the shared lane
    function (agx_node_sweep_lane) runs the same edges on the device; and the two-variant groups in a tile that holds a three-variant position elsewhere."""
    W = window(IV)
    ps, want, psl = [], [], []
    for i, rev in enumerate((False, True)):
        x, M = 2048 + i * 1024 + 8, 10240 + i * 1000 + 2 * W
        ps += _group(x, [M, M + W, M - W, M + W + 1, M - (W + 1)], rev)
        what = "both sides at once%s" % (", reverse" if rev else "")
        want += [mates_are(x + Q, [(M + Q, 3), (M + Q + W + 1, 1), (M + Q - W - 1, 1)], what), tile_variants(x + Q, 3, 4, what + " (pass 1)")]
        psl.append(plain(x - 220, x + 5))
        # the high-side group two tiles on, with three variants SEP apart at the tile's last positions
        x2, M2 = x + 128 + 200, M + 3000
        ps += _group(x2, [M2, M2 + W, M2 - W, M2 + W + 1], rev) + [EU.end_at(x2 - 9, M2 + 1000 + v * SEP) for v in range(3)]
        want += [mates_are(x2 + Q, [(M2 + Q, 3), (M2 + Q + W + 1, 1)], what + ", beside three variants"),
                 ("%s: three variants elsewhere in the tile" % what, lambda o, s, x2=x2: (x2 - 9) // TILE == (x2 + Q) // TILE and len(ids_at(o, x2 - 9)) == 3)]
    want.append(("pass 1 takes tiles and keeps them", lambda o, s: tiles_beyond(o, 2) >= 4 and tiles_beyond(o, 4) == 0))
    return Case("c_mid", "C", WinUnit(16 * 1024, ps, psl=psl), want, reprune=(2,))


def case_c_small():
    """C with small mate positions: variant 0's mate position minus W is 0, and is negative (the device keeps it pre-subtracted in unsigned arithmetic: it wraps)."""
    W = window(IV)
    ps = _group(0, [W, 0, 2 * W, 2 * W + 1], False) + _group(100, [110, 100, 110 + W, 110 + W + 1], True)
    ps += _group(300, [310 + W, 310, 309], False)       # the low edge: 310 lies W below variant 0's mate and joins, 309 does not
    want = [mates_are(Q, [(W + Q, 3), (2 * W + 1 + Q, 1)], "variant 0's mate at W + q, arrivals down to mate position q"),
            mates_are(105, [(115, 3), (115 + W + 1, 1)], "variant 0's mate below W"),
            mates_are(300 + Q, [(310 + W + Q, 2), (309 + Q, 1)], "low edge"),
            record_kind(Q, LU.KIND_ONE, False, "small"), record_kind(105, LU.KIND_ONE, True, "small")]
    return Case("c_small", "C", WinUnit(4096, ps, psl=[plain(1024, 1324)]), want)


def case_c_nomate():
    """C's `none` terms: an arrival without a mate position (the other mate's soft clip) against a variant 0 that has one, and the reverse: a variant 0 without one takes
    every arrival (the device's v0_mwin = NONE)."""
    ps, want, psl = [], [], []
    for i, rev in enumerate((False, True)):
        x, M = 1024 + i * 1024 + 8, 6000 + i * 1000
        nomate = pair(x, M + 30, other_cigar="30S70M", rev=rev)      # indices 0..29 have no mate position; index q >= 30 has M + q
        ps += [nomate, pair(x, M, rev=rev), pair(x, M + SEP, rev=rev)]
        what = "no mate first%s" % (", reverse" if rev else "")
        want += [mates_are(x + Q, [(NONE, 3)], what), mates_are(x + 50, [(M + 50, 2), (M + SEP + 50, 1)], what + " (where it has one)")]
        x += 512
        ps += [pair(x, M, rev=rev), pair(x, M + 30, other_cigar="30S70M", rev=rev), pair(x, M + SEP, rev=rev)]
        what = "mate first%s" % (", reverse" if rev else "")
        want += [mates_are(x + Q, [(M + Q, 2), (M + SEP + Q, 1)], what), no_general(x + Q, what)]
        psl += [plain(x - 512 - 220, x - 512 + 5), plain(x - 220, x + 5)]
    return Case("c_nomate", "C", WinUnit(8192, ps, psl=psl), want)


# ---- clause B: the mate position's conti-mer ----------------------------------------------------------------------------------------------------------

GAP_B = 60      # contig-side gap of the contigs under the mates: positions d apart across it have contig offsets d + GAP_B apart


def _gapped(T, a, g, n_after=150, strand="+"):
    """A contig whose indices 0 .. a lie at T .. T + a and a + g .. at T + a ..: position T + a - 1 carries offset a - 1, T + a carries a + g."""
    return contig(a + g + n_after, [(0, T, a), (a + g, T + a, n_after)], strand)


def case_b_gap():
    """B alone decides: the mates lie on one contig, 65 and 66 positions apart (clause C passes: W = 125) on either side of a contig-side gap of 60, so their contig
    offsets are 125 and 126 apart, in both orders of arrival.  The contigs: '+', '-', one whose border lies 20 offsets in (variant 0's offset minus W wraps; before the
    contig starts variant 0 has no mate contig and the arrival has one, and the reverse), one under a second, plain contig (two conti-mers at the mate position:
    never the straight-line case)."""
    W = window(IV)
    assert 65 + GAP_B == W
    ps, want, psl = [], [], []
    spots = [("+ strand", 11000, 150, "+", False), ("- strand", 11600, 150, "-", False), ("border near the contig's start", 12200, 20, "+", False),
             ("two conti-mers at the mate position", 12800, 150, "+", True), ("+ strand, reverse reads", 13400, 150, "+", False)]
    i = 0
    for what, T, a, strand, two in spots:
        psl.append(_gapped(T, a, GAP_B, 300 - a if a < 100 else 150, strand))
        rev = "reverse" in what
        o1 = T + a - 70      # index q: the nearer mate at T + a - 70 + q (before the border for q < 70), the farther beyond it for q >= 5
        for d, first_far in ((65, False), (66, False), (65, True), (66, True)):
            x = 1024 + i * 384 + 8
            i += 1
            ps += _group(x, [o1 + d, o1] if first_far else [o1, o1 + d], rev)
            X = x + (60 if a < 100 else 40)
            sign = -1 if first_far else 1
            w = "%s, mates %d apart%s" % (what, d, ", the farther first" if first_far else "")
            n_keys = 2 if two else 1
            if d == 65:
                want.append(("%s: offsets 125 apart share variant 0 (coverage %d)" % (w, 2 * n_keys), lambda o, s, X=X, n=n_keys: cov_at(o, X) == [2 * n]))
            else:
                want.append(("%s: offsets 126 apart on one contig, mate positions 66 apart, make two variants" % w,
                             lambda o, s, X=X, sign=sign: len(ids_at(o, X)) == 2 and keys_at(o, X, 2)[0] == keys_at(o, X, 2)[1] != NONE and
                             keys_at(o, X, 3)[1] - keys_at(o, X, 3)[0] == sign * 126 and keys_at(o, X, 5)[1] - keys_at(o, X, 5)[0] == sign * 66))
            if a < 100 and not first_far:     # before the contig starts under the nearer mate: variant 0 has no mate contig, the arrival has one
                want.append(("%s: variant 0 without a mate contig takes the arrival that has one" % w, lambda o, s, x=x: keys_at(o, x + 20, 2) == [NONE] and cov_at(o, x + 20) == [2]))
            if a < 100 and first_far:
                want.append(("%s: variant 0 with a mate contig takes the arrival that has none" % w, lambda o, s, x=x: len(ids_at(o, x + 20)) == 1 and keys_at(o, x + 20, 2)[0] != NONE and cov_at(o, x + 20) == [2]))
            psl.append(plain(x - 220, x + 5))
    # the second conti-mer: a plain contig over the fourth spot, written behind the gapped one (conti-mers keep the contigs' order)
    psl.append(plain(12800 - 60, 12800 + 320, "-"))
    want.append(("two conti-mers under the fourth spot's mates", lambda o, s: int(o["graph"]["cm_count"][12800 + 100]) == 2))
    return Case("b_gap", "B", WinUnit(16 * 1024, ps, psl=psl), want, reprune=(2,))


def case_b_edge():
    """B on the edge side: a step x -> x + 1 between single variants whose STORED mate-side keys lie 125 (the edge stands) and 126 (it does not) offsets apart on one contig,
    inside a tile (the fused write of agx_node_write_lane) and on lane 63 (agx_edge_allowed in pass A).  x's key is stored by a read that ends on x (mate at m1), x + 1's by a
    read that skips x with a deletion (mate at m1 + 65 or m1 + 66, beyond the contig-side gap of 60); the read that steps from x to x + 1 has its mate between the two and is
    compatible with both (edge_units.case_boundary's refused step, on the window's edge)."""
    ps, want, psl, i = [], [], [], 0
    for what, lane in (("inside a tile", 30), ("lane 63", 63)):
        for d in (65, 66):
            x, T = 2048 + i * 1024 + 512 + lane, 8192 + i * 600
            i += 1
            psl.append(_gapped(T, 150, GAP_B))
            m1 = T + 150 - 33
            ps += [EU.end_at(x, m1), EU.dele(x - 1, [1], m1 + d - 1, q=60), EU.span(x, m1 + 30)]
            stands = d + GAP_B <= window(IV)
            w = "%s, stored mate offsets %d apart" % (what, d + GAP_B)
            want.append(("%s: single variants on one mate contig, the edge %s" % (w, "stands" if stands else "is refused"),
                         lambda o, s, x=x, d=d, st=stands: len(ids_at(o, x)) == 1 and len(ids_at(o, x + 1)) == 1 and keys_at(o, x, 2)[0] == keys_at(o, x + 1, 2)[0] != NONE and
                         keys_at(o, x + 1, 3)[0] - keys_at(o, x, 3)[0] == d + GAP_B and keys_at(o, x + 1, 5)[0] - keys_at(o, x, 5)[0] == d and edge(o, x, 0, x + 1, 0) == st))
            want.append(("%s: a read steps from %d to %d" % (w, x, x + 1), lambda o, s, x=x: cov_at(o, x) == [1] and cov_at(o, x + 1) == [2]))
            want.append(tile_variants(x, 1, 2, w))
            psl.append(plain(x - 320, x - 96))
    want += [("pass A refuses a step on lane 63", lambda o, s: s["edges"]["a_refused"] >= 1), ("pass A writes a step on lane 63", lambda o, s: s["edges"]["a_written"] >= 1)]
    return Case("b_edge", "B", WinUnit(12 * 1024, ps, psl=psl), want)


# ---- the consensus base's ties ------------------------------------------------------------------------------------------------------------------------

TIES = ("AC", "AG", "AT", "AN", "CG", "CT", "CN", "GT", "GN", "TN")


def case_ties():
    """Not a window, but a rule of the same kind (AG:1944-1952): a node whose votes tie takes the first of A, C, G, T, N.  Two reads vote for every pair of bases at positions of
    their own, in both file orders and on both strands, behind a contig whose extension walks through them."""
    ps, want, psl = [], [], []
    for i, (rev, swap) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        x = 1024 + i * 512 + 8
        b1, b2 = {10 + 3 * j: t[0] for j, t in enumerate(TIES)}, {10 + 3 * j: t[1] for j, t in enumerate(TIES)}
        if swap:
            b1, b2 = b2, b1
        ps += [pair(x, x + OFF, rev=rev, bases=b1), pair(x, x + OFF, rev=rev, bases=b2)]
        psl.append(plain(x - 220, x + 5))
        for j, t in enumerate(TIES):
            cols = ["ACGTN".index(c) + 1 for c in t]
            want.append(("%s tie at %d" % (t, x + 10 + 3 * j), lambda o, s, X=x + 10 + 3 * j, cols=cols: len(ids_at(o, X)) == 1 and
                         [int(v) for v in o["graph"]["node_cnt"][ids_at(o, X)[0], 1:]] == [1 if c in cols else 0 for c in range(1, 6)]))
    want.append(("the extension spells the tied positions", lambda o, s: len(o["extended"]) > 4 * 300))
    return Case("ties", "T", WinUnit(4096, ps, psl=psl), want)



# ---- clause A: the position's own contig offset --------------------------------------------------------------------------------------------------------

def _twice(s0, n, D):
    """One contig placed twice: at s0 .. s0 + n, and with its first 30 bases at s0 - n and the rest D positions before where the first placement has them: positions
    s0 + i carry the contig's offsets i and i + D."""
    return contig(n, [(0, s0, n)], more=[[(0, s0 - n, 30), (30, s0 + 30 - D, n - 30)]])


def case_a_node():
    """A on the node side (agx_compatible, candidate keys X-major): positions that carry two conti-mers of one contig 25 and 26 offsets apart.  At 25 the second candidate
    key matches the first one's variant (it counts twice); at 26 it makes its own.  At 26 the steps x -> x + 1 have two variants on either side: the edge from the
    second variant of x (offset i + 26) to the first of x + 1 (offset i + 1) is 25 apart and stands, the one from the first to the second is 27 apart and does not."""
    ps, want, psl = [], [], []
    for s0, D in ((3072, 25), (3072 + 2048, 26), (3072 + 4096, 24)):
        psl.append(_twice(s0, 300, D))
        ps += [pair(s0 + 100, s0 + 100 + OFF)] * 2
        X = s0 + 110
        want.append(("two conti-mers at %d" % X, lambda o, s, X=X: int(o["graph"]["cm_count"][X]) == 2))
        if D <= EP25:
            want.append(("offsets %d apart: one variant, counted once per candidate key" % D, lambda o, s, X=X: cov_at(o, X) == [4] and keys_at(o, X, 1) == [110]))
        else:
            want.append(("offsets 26 apart: two variants", lambda o, s, X=X: cov_at(o, X) == [2, 2] and keys_at(o, X, 1) == [110, 136] and keys_at(o, X, 0)[0] == keys_at(o, X, 0)[1]))
            want.append(("offsets 26 apart: the edge 25 apart stands, the edge 27 apart does not",
                         lambda o, s, X=X: edge(o, X, 0, X + 1, 0) and edge(o, X, 1, X + 1, 1) and edge(o, X, 1, X + 1, 0) and not edge(o, X, 0, X + 1, 1)))
    return Case("a_node", "A", WinUnit(10 * 1024, ps, psl=psl), want, reprune=(3,))


def _a_region(i, lane):
    return 2048 + i * 1024 + 512 + lane


def case_a_edge():
    """A on the edge side: a step x -> x + 1 across a PSL block border whose contig-side gap makes the two stored offsets differ by exactly 25 (the edge stands) and 26 (it
    does not), on '+' and '-' contigs; the step inside a tile with single variants (the fused write of agx_node_write_lane), on lane 63 (agx_edge_allowed in pass A),
    behind a two-variant source on lane 63 and before a two-variant target (agx_resolve / agx_key_compatible in pass B), inside a tile with five variants elsewhere
    (pass 2), and as a deletion's jump of 25 and 26 positions over one plain contig (pass J)."""
    ps, want, psl, i = [], [], [], 0

    def offsets(x, what, g):
        return ("%s: the stored contig offsets of %d and %d are %d apart on one contig" % (what, x, x + 1, g + 1),
                lambda o, s: keys_at(o, x + 1, 1)[0] - keys_at(o, x, 1)[0] == g + 1 and keys_at(o, x, 0)[0] == keys_at(o, x + 1, 0)[0] != NONE)

    Z = 2048 + 16 * 1024      # every read's mate lies in a zone behind the last region, where no contig is: clause A alone decides
    for what, lane, strand, extra in (("inside a tile", 30, "+", None), ("inside a tile, - strand", 30, "-", None), ("lane 63", 63, "+", None), ("lane 63, - strand", 63, "-", None),
                                      ("two-variant source on lane 63", 63, "+", "src"), ("two-variant target", 63, "+", "dst"), ("pass-2 tile", 30, "+", "big")):
        for g in (EP25 - 1, EP25):
            x, MO = _a_region(i, lane), Z - (2048 + i * 1024)
            i += 1
            psl.append(_gapped(x - 149, 150, g, 150, strand))
            w = "%s, gap %d" % (what, g)
            want.append(offsets(x, w, g))
            stands = g + 1 <= EP25
            verdict = "stands" if stands else "is refused"
            if extra == "src":      # (edge_units.case_boundary's multi -> single: the second variant comes from a read that ends on x)
                ps += [EU.end_at(x, x + MO), EU.end_at(x, x + MO + SEP), EU.span(x, x + MO)] + EU.cover(x + 1, x + 200, MO)
                want.append(("%s: the first variant's edge %s" % (w, verdict), lambda o, s, x=x, st=stands: len(ids_at(o, x)) == 2 and len(ids_at(o, x + 1)) == 1 and edge(o, x, 0, x + 1, 0) == st))
                want.append(EU_slow("%s: a register context of pass B" % w, x=x, who=1, n=2, n1=1, reg=1, allowed=lambda a, st=stands: (a & 1 == 1) == st))
            elif extra == "dst":    # (single -> multi)
                ps += EU.cover(x - 200, x + 1, MO) + [EU.start_at(x + 1, x + 1 + MO), EU.start_at(x + 1, x + 1 + MO + SEP), EU.span(x, x + MO)]
                want.append(("%s: the edge to the first variant %s" % (w, verdict), lambda o, s, x=x, st=stands: len(ids_at(o, x)) == 1 and len(ids_at(o, x + 1)) == 2 and edge(o, x, 0, x + 1, 0) == st))
                want.append(EU_slow("%s: a register context of pass B" % w, x=x, who=1, n=1, n1=2, reg=1, allowed=lambda a, st=stands: (a & 1 == 1) == st))
            else:
                ps += EU.cover(x - 200, x + 200, MO)
                want.append(("%s: single variants, the edge %s" % (w, verdict), lambda o, s, x=x, st=stands: len(ids_at(o, x)) == 1 and len(ids_at(o, x + 1)) == 1 and edge(o, x, 0, x + 1, 0) == st))
                if extra == "big":
                    ps += [EU.end_at(x - 12, x - 12 + MO + v * SEP) for v in range(1, 6)]
                    want.append(tile_variants(x, 5, 64, w))
                else:
                    want.append(tile_variants(x, 1, 1, w))
    want += [("pass A refuses a step on lane 63", lambda o, s: s["edges"]["a_refused"] >= 2), ("pass A writes a step on lane 63", lambda o, s: s["edges"]["a_written"] >= 2)]
    # pass J: deletions of 24 and 25 bases over a plain contig: the jump's two offsets are 25 and 26 apart
    for d in (EP25 - 1, EP25):
        x, MO = _a_region(i, 20), Z - (2048 + i * 1024)
        i += 1
        psl.append(plain(x - 150, x + 250))
        ps += EU.cover(x - 150, x + 200, MO) + [EU.dele(x, [d], x + MO)]
        stands = d + 1 <= EP25
        want.append(("jump of %d: offsets %d apart, the edge %s" % (d + 1, d + 1, "stands" if stands else "is refused"),
                     lambda o, s, x=x, d=d, st=stands: keys_at(o, x + d + 1, 1)[0] - keys_at(o, x, 1)[0] == d + 1 and edge(o, x, 0, x + d + 1, 0) == st))
        want.append(("pass J looks at the jump of %d" % (d + 1), lambda o, s, x=x, d=d: any(int(j["x"]) == x and int(j["xs"]) == x + d + 1 for j in s["jsteps"])))
        want.append(("pass J %s the jump of %d" % ("inserts" if stands else "does not insert", d + 1),
                     lambda o, s, x=x, d=d, st=stands: any(int(j["x"]) == x and int(j["xs"]) == x + d + 1 for j in s["jins"]) == st))
    assert i == 16
    want.append(("pass 2 takes the tiles with six variants", lambda o, s: tiles_beyond(o, 4) >= 2))
    return Case("a_edge", "A", WinUnit(Z + 2560, ps, psl=psl), want, reprune=(2,))


def EU_slow(desc, **want):
    what, fn = EU.slow_where(desc, **want)
    return (what, lambda o, s: fn(s))


def cases():
    return [case_c_lean(), case_c_lean(20), case_c_general(), case_c_mid(), case_c_small(), case_c_nomate(), case_b_gap(), case_b_edge(), case_a_node(), case_a_edge(), case_ties()]
