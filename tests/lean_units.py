"""Hand-made units that pin pass 0 of the node sweep (agx_sweep_tile_lean, agx_kernels.hip) arm by arm.

A unit is a seeded genome, a list of pairs — each mate with its leftmost aligned position, CIGAR and strand, plus bases overridden at chosen
read indices — and optionally contigs with their PSL lines.  write_unit() writes the tmp/ files the loaders read, the way
conftest.write_pileup_unit does.  Every case below is a function of this module, so the CPU twin (tests/test_lean_sweep_cases.py) and the GPU
file (tests/test_gpu_lean_sweep.py) build exactly the same inputs, and each case names the lean record shapes (agx_lrec, agx_core.h) it is
there for: check_shapes() reads them from the serial executor's records (hostsim.sim.run(..., records=True)), so a case cannot silently stop
covering its arm.  The oracle decides what is correct; nothing here works out expected counts.

Read index q runs along the CIGAR in reference orientation (soft clips and insertions included), in both mates alike (the loaders' model:
index q of mate 1 pairs with index q of mate 2).  A reverse-strand mate's read is stored reverse-complemented, as a sequencer reports it.
"""
import os
import random

K, IV = 5, 50                # every case runs with k = 5, insertVariation = 50, coverage 1
L = 100                      # read length
W = 2 * IV + 25              # mate positions further apart than this make node variants of their own (AG:1296-1307)
TILE = 64

KIND_GENERAL, KIND_ONE, KIND_ONEX, KIND_TWO = 0, 1, 2, 3
LF_AREV, LF_BN1, LF_BN2, LF_JUMP1, LF_MID, LF_JUMP2 = 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def _cigar_ops(cigar):
    ops, num = [], ""
    for c in cigar:
        if c.isdigit():
            num += c
        else:
            ops.append((int(num), c))
            num = ""
    return ops


def cigar_len(cigar):
    return sum(n for n, op in _cigar_ops(cigar) if op in "MIS")


class Mate:
    """pos: 0-based reference position of the first aligned base (SAM POS - 1)."""

    def __init__(self, pos, cigar="%dM" % L, rev=False):
        self.pos, self.cigar, self.rev = pos, cigar, rev


class Pair:
    """bases: {read index: base} written into BOTH mates' reads (only the left mate's bases are ever read)."""

    def __init__(self, m1, m2, bases=None):
        self.m1, self.m2, self.bases = m1, m2, dict(bases or {})


def pair(left, other, left_cigar="%dM" % L, other_cigar="%dM" % L, rev=False, left_is_mate2=False, bases=None):
    """A pair whose left mate (the one whose indices emit the arrivals) lies at `left` on strand `rev`, its other mate at `other` on the opposite strand."""
    a, b = Mate(left, left_cigar, rev), Mate(other, other_cigar, not rev)
    return Pair(b, a, bases) if left_is_mate2 else Pair(a, b, bases)


class Unit:
    def __init__(self, genome_len, pairs, contigs=(), seed=11):
        """contigs: (start, end, strand) — the contig is genome[start:end] (reverse-complemented for '-'), aligned there by one PSL block."""
        self.genome_len, self.pairs, self.contigs, self.seed = genome_len, list(pairs), list(contigs), seed


def _read_of(g, m, bases, rnd):
    seq, x = [], m.pos
    for n, op in _cigar_ops(m.cigar):
        if op == "M":
            seq.append(g[x:x + n])
            x += n
        elif op == "D":
            x += n
        elif op in "IS":
            seq.append("".join(rnd.choice("ACGT") for _ in range(n)))
    assert x <= len(g), "alignment beyond the end of the genome"
    s = list("".join(seq))
    for q, c in bases.items():
        s[q] = c
    s = "".join(s)
    return revcomp(s) if m.rev else s


def _flag(me, mate, first):
    return 1 | 2 | (64 if first else 128) | (16 if me.rev else 0) | (32 if mate.rev else 0)


def write_unit(unit, run):
    """Writes run/tmp/{_genome.0.fa, _contigs.fa, _contigs_genome.0.psl, _reads.fa, _reads_genome.0.bowtie}; returns the tmp/ directory."""
    rnd = random.Random(unit.seed)
    tmp = os.path.join(run, "tmp")
    os.makedirs(tmp, exist_ok=True)
    G = unit.genome_len
    g = "".join(rnd.choice("ACGT") for _ in range(G))
    with open(os.path.join(tmp, "_genome.0.fa"), "w") as f:
        f.write(">0\n" + "".join(g[i:i + 60] + "\n" for i in range(0, G, 60)))
    with open(os.path.join(tmp, "_contigs.fa"), "w") as cf, open(os.path.join(tmp, "_contigs_genome.0.psl"), "w") as pf:
        for i, (s, e, strand) in enumerate(unit.contigs):
            n, name = e - s, "%d.%d" % (i, i)
            seq = g[s:e] if strand == "+" else revcomp(g[s:e])
            cf.write(">%s\n%s\n" % (name, "".join(seq[j:j + 60] + "\n" for j in range(0, n, 60)).rstrip("\n")))
            pf.write("%d\t0\t0\t0\t0\t0\t0\t0\t%s\t%s\t%d\t0\t%d\t0\t%d\t%d\t%d\t1\t%d,\t0,\t%d,\n" % (n, strand, name, n, n, G, s, e, n, s))
    cache = {}
    with open(os.path.join(tmp, "_reads.fa"), "w") as rf, open(os.path.join(tmp, "_reads_genome.0.bowtie"), "w") as sf:
        for i, p in enumerate(unit.pairs):
            assert cigar_len(p.m1.cigar) == cigar_len(p.m2.cigar), "mates of one pair have different CIGAR lengths"
            key = (p.m1.pos, p.m1.cigar, p.m1.rev, p.m2.pos, p.m2.cigar, p.m2.rev, tuple(sorted(p.bases.items())))
            if key not in cache:      # (identical pairs — the pile-ups of tens of thousands — share their text)
                r1, r2 = _read_of(g, p.m1, p.bases, rnd), _read_of(g, p.m2, p.bases, rnd)
                cache[key] = ("%s\n>{0}\n%s\n" % (r1, r2),
                              "\t%d\t0\t%d\t42\t%s\t=\t%d\t0\t*\t*\n" % (_flag(p.m1, p.m2, True), p.m1.pos + 1, p.m1.cigar, p.m2.pos + 1),
                              "\t%d\t0\t%d\t42\t%s\t=\t%d\t0\t*\t*\n" % (_flag(p.m2, p.m1, False), p.m2.pos + 1, p.m2.cigar, p.m1.pos + 1))
            reads, s1, s2 = cache[key]
            rf.write(">%d\n" % i + reads.replace("{0}", str(i)))
            sf.write("%d%s%d%s" % (i, s1, i, s2))
    return tmp


# ---- lean records as the serial executor reports them (sim.run(..., records=True)) ---------------------------------------------------

def fields(recs):
    """The lean records' geometry (agx_lean_decode) as arrays: kind, rev, lo1, e1 (last lane of piece 1), lo2, e2, the AGX_LF_* flags, js (jstar), len."""
    import numpy as np
    g = recs["geo"].astype(np.int64)
    lo1, lo2 = g & 63, (g >> 12) & 63
    return {"tile": recs["tile"].astype(np.int64), "kind": g >> 30, "rev": (g & LF_AREV) != 0, "lo1": lo1, "e1": lo1 + ((g >> 6) & 63), "lo2": lo2, "e2": lo2 + ((g >> 18) & 63),
            "bn1": (g & LF_BN1) != 0, "bn2": (g & LF_BN2) != 0, "jump1": (g & LF_JUMP1) != 0, "mid": (g & LF_MID) != 0, "jump2": (g & LF_JUMP2) != 0,
            "qoff1": recs["qoff1"].astype(np.int64), "qoff2": recs["qoff2"].astype(np.int64), "boff1": recs["boff1"].astype(np.int64), "boff2": recs["boff2"].astype(np.int64),
            "js": recs["lenjs"].astype(np.int64) >> 16, "len": recs["lenjs"].astype(np.int64) & 0xFFFF}


def count(recs, **want):
    """Entries whose fields equal the given values (a callable value is a predicate on the field's array)."""
    import numpy as np
    f = fields(recs)
    m = np.ones(len(recs), bool)
    for k, v in want.items():
        m &= v(f[k]) if callable(v) else (f[k] == v)
    return int(m.sum())


def check_shapes(case, out):
    """Asserts that every record shape the case names occurs; out = sim.run(..., records=True)."""
    for what, want in case.shapes:
        if what == "tile_len":
            for n in want:
                assert n in set(out["tile_len"].tolist()), "%s: no tile list of %d entries" % (case.name, n)
        else:
            assert count(out["records"], **want) >= 1, "%s: no lean record with %s (%s)" % (case.name, want, what)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, group, unit, shapes, stats=None, slow=False):
        """shapes: [(description, {field: value})] or ("tile_len", [n, ..]); stats: what the device's pass statistics must say — a dict of
        name -> value or predicate, for the engine's n_mid_tiles / n_big_tiles; the executor's pass 0 gives up on a tile where the device's n_mid_tiles counts it."""
        self.name, self.group, self.unit, self.shapes, self.stats, self.slow = name, group, unit, shapes, stats or {}, slow


def _regions(specs, gap=1024, first=1024):
    """Places one group of pairs per region, `gap` positions apart: specs = [(offset inside a tile, fn(x0) -> [Pair])]; returns the pairs."""
    out = []
    for i, (lane, fn) in enumerate(specs):
        out += fn(first + i * gap + lane)
    return out


def _both_strands(lane, fn):
    return [(lane, lambda x: fn(x, False)), (lane, lambda x: fn(x, True))]


def case_one():
    """A. kind ONE: both strands, left mate = mate 1 and = mate 2; pieces that start on lane 0 and end on lane 63; jstar (the K2ONLY arrival: index L - k) on lane 63 and on lane 0
    of the next tile."""
    specs = []
    for rev in (False, True):
        for m2 in (False, True):
            specs.append((40, lambda x, rev=rev, m2=m2: [pair(x, x + 400, rev=rev, left_is_mate2=m2)] * 3))
        specs.append((63 - (L - K), lambda x, rev=rev: [pair(x, x + 400, rev=rev)] * 2))          # jstar on lane 63
        specs.append((64 - (L - K), lambda x, rev=rev: [pair(x, x + 400, rev=rev)] * 2))          # jstar on lane 0 of the next tile
    unit = Unit(16 * 1024, _regions(specs))
    sh = [("forward", {"kind": KIND_ONE, "rev": False}), ("reverse", {"kind": KIND_ONE, "rev": True}),
          ("starts on lane 0", {"kind": KIND_ONE, "lo1": 0}), ("ends on lane 63", {"kind": KIND_ONE, "e1": 63})]
    for rev in (False, True):
        sh += [("K2ONLY on lane 63", {"kind": KIND_ONE, "rev": rev, "e1": 63, "boff2": 63}),
               ("K2ONLY on lane 0 of the next tile: the tile before sees none", {"kind": KIND_ONE, "rev": rev, "e1": 63, "boff2": 64}),
               ("K2ONLY alone on lane 0", {"kind": KIND_ONE, "rev": rev, "lo1": 0, "e1": 0, "boff2": 0})]
    return Case("one", "A", unit, sh)


def case_unit_end(m, extra):
    """A. the unit's last position is a left mate's last arrival (96M4S: jstar = index 95, the last aligned one), unit length 64 m + extra."""
    G = 64 * m + extra
    x = G - 1 - (L - K)
    pairs = [pair(1000, 1400), pair(1000, 1400, rev=True)] + [pair(x, x, "96M4S", "96M4S"), pair(x, x, "96M4S", "96M4S", rev=True)] * 2
    lane = (G - 1) % 64
    return Case("unit_end_%d" % extra, "A", Unit(G, pairs), [("last arrival on the unit's last lane", {"kind": KIND_ONE, "tile": (G - 1) // 64, "e1": lane, "boff2": lane})])


def case_onex():
    """B. kind ONEX: BN1 (the other mate has no position under the piece: a soft clip; an insertion) and JUMP1 (a left-mate deletion at the piece's end, on lane 63 and 62)."""
    specs = []
    specs += _both_strands(40, lambda x, rev: [pair(x, x + 400 - 30, other_cigar="30S70M", rev=rev)] * 2)              # piece of tile t: indices 0..23, no mate position
    specs += _both_strands(40, lambda x, rev: [pair(x, x + 400, other_cigar="2M30I68M", rev=rev)] * 2)                 # indices 2..31 inserted in the other mate
    specs += _both_strands(24, lambda x, rev: [pair(x, x + 400, left_cigar="40M10D60M", rev=rev)] * 2)                 # index 39 on lane 63
    specs += _both_strands(23, lambda x, rev: [pair(x, x + 400, left_cigar="40M10D60M", rev=rev)] * 2)                 # index 39 on lane 62
    sh = []
    for rev in (False, True):
        sh += [("BN1", {"kind": KIND_ONEX, "rev": rev, "bn1": True, "lo1": 40, "e1": 63}),
               ("JUMP1 on lane 63", {"kind": KIND_ONEX, "rev": rev, "jump1": True, "e1": 63, "bn1": False}),
               ("JUMP1 on lane 62", {"kind": KIND_ONEX, "rev": rev, "jump1": True, "e1": 62, "bn1": False})]
    return Case("onex", "B", Unit(16 * 1024, _regions(specs)), sh)


def case_two():
    """C. kind TWO: a left-mate insertion (qoff changes), a left-mate deletion (JUMP1, empty lanes between the pieces), a break of the other mate (boff changes), MID (an
    insertion of the other mate), BN2 (its trailing soft clip), JUMP2 (a left-mate deletion behind a break of the other mate); each on both strands."""
    specs = []
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, left_cigar="50M3I47M", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, left_cigar="40M5D60M", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, other_cigar="50M5D50M", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, other_cigar="50M5I45M", rev=rev)] * 2)
    specs += _both_strands(32, lambda x, rev: [pair(x, x + 400, other_cigar="80M20S", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, left_cigar="60M10D40M", other_cigar="40M5D60M", rev=rev)] * 2)
    sh = []
    for rev in (False, True):
        sh += [("left-mate insertion", {"kind": KIND_TWO, "rev": rev, "e1": 49, "lo2": 50, "qoff2": lambda v: v != 0, "jump1": False}),
               ("left-mate deletion", {"kind": KIND_TWO, "rev": rev, "e1": 39, "lo2": 45, "jump1": True}),
               ("other-mate break", {"kind": KIND_TWO, "rev": rev, "e1": 49, "lo2": 50, "qoff1": 0, "qoff2": 0, "mid": False, "bn2": False, "jump1": False}),
               ("MID", {"kind": KIND_TWO, "rev": rev, "mid": True, "e1": 49, "lo2": 55}),
               ("BN2", {"kind": KIND_TWO, "rev": rev, "bn2": True, "e1": 47, "lo2": 48}),
               ("JUMP2", {"kind": KIND_TWO, "rev": rev, "jump2": True, "e2": 59})]
    return Case("two", "C", Unit(16 * 1024, _regions(specs)), sh)


def case_general():
    """D. kind GENERAL: three pieces in one tile, a read insertion next to a reference gap (CHAIN arrivals), a mate of more than AGX_LEAN_MAXRUNS runs; each on both strands
    (a reverse-strand GENERAL record counted its votes from the wrong end of the read in r06's first form)."""
    specs = []
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, left_cigar="30M2I20M3D48M", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, left_cigar="40M3I5D57M", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, other_cigar="20M1D20M1D20M1D40M", rev=rev)] * 2)
    specs += _both_strands(0, lambda x, rev: [pair(x, x + 400, left_cigar="20M1D20M1D20M1D40M", rev=rev)] * 2)
    sh = [("general, forward", {"kind": KIND_GENERAL, "rev": False}), ("general, reverse", {"kind": KIND_GENERAL, "rev": True})]
    return Case("general", "D", Unit(16 * 1024, _regions(specs)), sh)


def case_votes():
    """E. five left mates that disagree at read indices 20 and 50 (and agree with ten more): all five vote fields non-zero at one position, on both strands."""
    def fn(x, rev):
        ps = []
        for i, c in enumerate("ACGTN" * 3):
            ps.append(pair(x, x + 400, rev=rev, bases={20: c, 50: "ACGTN"[(i + 2) % 5]}))
        return ps
    specs = _both_strands(40, fn)
    return Case("votes", "E", Unit(8 * 1024, _regions(specs)), [("forward", {"kind": KIND_ONE, "rev": False}), ("reverse", {"kind": KIND_ONE, "rev": True})])


FLUSH_LENGTHS = (1, 2, 3, 61, 62, 63, 64, 123, 124, 125, 128, 190)      # (the first entry of a list stores variant 0 outside the register counters: only from 128 on
#  does a later chunk of 64 entries — a flush every 64 instead of 62 — bring 64 votes of one base into a 6-bit field)


def case_flush():
    """E. lists of 1, 2, 3, 61, 62, 63, 64, 123, 124, 125, 128 and 190 identical entries (the register counters are flushed every 62 entries), forward and reverse pile-ups side by side."""
    specs = []
    for n in FLUSH_LENGTHS:
        specs.append((0, lambda x, n=n: [pair(x, x + 400)] * n))
        specs.append((0, lambda x, n=n: [pair(x, x + 400, rev=True)] * n))
    return Case("flush", "E", Unit(28 * 1024, _regions(specs)), [("tile_len", list(FLUSH_LENGTHS))])


def case_packed(n):
    """F. one tile list of n identical entries whose left mates all read A at index 10, G at 30 and N at 50: coverage and the high halves of the packed counter words (A, G, N)
    reach n at some position.  65 535 is the most pass 0 keeps; 65 536 goes to pass 1."""
    bases = {10: "A", 30: "G", 50: "N"}
    return Case("packed_%d" % n, "F", Unit(4096, [pair(1024, 1500, bases=bases)] * n), [("tile_len", [n])],
                stats={"n_mid_tiles": 0} if n <= 65535 else {"n_mid_tiles": lambda v: v >= 1}, slow=True)


def case_variants():
    """G. two node variants at a position (pass 0 keeps the tile), an arrival compatible with variant 1 only and one compatible with both, with variant 1's first arrival early and
    last in the list; a position whose first arrival is K2ONLY followed by K1 arrivals of the same key."""
    def early(x):
        return [pair(x, x + 2000), pair(x, x + 2000 + W + 5), pair(x, x + 2000), pair(x, x + 2000 + W // 2), pair(x, x + 2000 + W + 75), pair(x, x + 2000)]

    def late(x):
        return [pair(x, x + 2000), pair(x, x + 2000 + W // 2), pair(x, x + 2000), pair(x, x + 2000 + W + 75), pair(x, x + 2000 + W + 5)]

    def k2first(x):
        return [pair(x, x + 2000)] + [pair(x + 10, x + 2010)] * 3

    specs = []
    for fn in (early, late, k2first):
        specs += [(8, fn), (8, lambda x, fn=fn: [pair(p.m1.pos, p.m2.pos, rev=True) for p in fn(x)])]
    return Case("variants", "G", Unit(24 * 1024, _regions(specs, gap=3072)), [("forward", {"kind": KIND_ONE, "rev": False}), ("reverse", {"kind": KIND_ONE, "rev": True})],
                stats={"n_mid_tiles": 0})


def case_third_variant():
    """G. a third variant at the positions of one left mate: pass 1 takes the tile (and keeps it)."""
    pairs = [pair(1000, 3000 + i * 300, rev=(i == 1)) for i in range(3)] * 2
    return Case("third_variant", "G", Unit(8192, pairs), [("forward", {"kind": KIND_ONE, "rev": False})], stats={"n_mid_tiles": lambda v: v >= 1, "n_big_tiles": 0})


def case_contimers():
    """G. mate positions that carry two conti-mers (overlapping contigs, one on each strand, through the PSL) and positions that carry one."""
    pairs = [pair(1000, 3000), pair(1000, 3000, rev=True), pair(1000, 3000 + W + 20), pair(1010, 3010)] * 2
    contigs = [(2700, 3350, "+"), (3000, 3700, "-"), (900, 1400, "+")]
    return Case("contimers", "G", Unit(8192, pairs, contigs), [("forward", {"kind": KIND_ONE, "rev": False})])


def cases(slow=True):
    out = [case_one(), case_unit_end(40, 0), case_unit_end(40, 1), case_unit_end(40, 63), case_onex(), case_two(), case_general(), case_votes(), case_flush(),
           case_variants(), case_third_variant(), case_contimers()]
    if slow:
        out += [case_packed(65535), case_packed(65536)]
    return out
