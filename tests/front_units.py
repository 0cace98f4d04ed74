"""Hand-made units that pin the FRONT of a build — the kernels that expand the upload forms (agx_k_expand_runs, agx_k_cm_layout, agx_k_cm_fill, agx_k_expand_codes,
agx_k_patch_codes, agx_k_expand_rows, agx_k_expand_ref, agx_k_patch_ref), agx_k_hit_prep, the scan of the tile histogram, agx_k_tile_fill in both forms, agx_k_bin_fill and
agx_k_tile_sort (agx_kernels.hip) — edge by edge.

The units are lean_units.Unit's (any CIGAR, any read length), plus two things a case may ask for: further hits of a pair (`more`: the rule of AG:1650-1655 drops a later hit
that lands within a read length of an earlier one) and edits of the files once they are written (`post`: the unit sequence's other bytes).  The CPU twin
(tests/test_front_cases.py) and the GPU file (tests/test_gpu_front.py) build exactly the same inputs, and every case names the arm it is there for as predicates on a View —
the serial executor's front (hostsim.sim.run(..., front=True)) and the plain model of tests/front_model.py over it: check_arms() asserts them, so a case cannot silently
stop reaching its arm.  What the DEVICE must report besides (which forms it used, how often it built) is in Case.device.  The oracle decides whether graph and files are
right; the model and the executor decide the arrays; nothing here works out expected values.

The hits of every unit here are the line pairs of its alignment file in order (none fails the identity filter), and the left mate of every pair is the one at the lower
position (or mate 1 where both lie at the same), so a hit's place in the staging's order is known even where the hit is skipped: left_x().
"""
import os

import numpy as np

import front_model as FM
import lean_units as LU
from lean_units import K, Unit, pair

TILE = 64
IUPAC = "RYKMSWBDHVN"


def P(x, L=100, cigar=None, gap=400, other_cigar=None, **kw):
    """A pair of reads of length L whose left mate lies at x, the other one `gap` further on."""
    return pair(x, x + gap, left_cigar=cigar or "%dM" % L, other_cigar=other_cigar or "%dM" % L, **kw)


class Case:
    def __init__(self, name, group, unit, L, arms, more=None, post=None, device=None, row_diff=False):
        """arms: [(description, fn(View) -> bool)].  more: {pair index: [(left, other), ..]} further hits of that pair, written behind its first.  post: fn(tmp) edits the
        written files.  device: {name: value or predicate} the engine must report in EVERY upload form — names of Unit.front() or Unit.stats(); the forms' own switches
        (tiled, rows_diffed, ref_packed, swept_windows) are asserted per form by the GPU file.  row_diff: the case is there for agx_k_expand_rows: under AGX_ROW_DIFF=1 the
        device must have taken the rows as differences, some of them explicit."""
        self.name, self.group, self.unit, self.L, self.arms, self.more, self.post, self.device, self.row_diff = name, group, unit, L, arms, dict(more or {}), post, dict(device or {}), row_diff


def hits_of(case):
    """(pair index, first aligned position of the left mate) per hit, in file order."""
    out = []
    for i, p in enumerate(case.unit.pairs):
        out.append((i, min(p.m1.pos, p.m2.pos)))
        for left, other in case.more.get(i, ()):
            out.append((i, min(left, other)))
    return out


def left_x(case):
    return {h: x for h, (_, x) in enumerate(hits_of(case))}


def genome_of(tmp):
    return "".join(open(os.path.join(tmp, "_genome.0.fa")).read().split("\n")[1:])


def write_genome(tmp, seq):
    with open(os.path.join(tmp, "_genome.0.fa"), "w") as f:
        f.write(">0\n" + "".join(seq[i:i + 60] + "\n" for i in range(0, len(seq), 60)))


def write_unit(case, run):
    """The case's tmp/ files: lean_units.write_unit, then the further hits of its pairs, then its edits."""
    tmp = LU.write_unit(case.unit, run)
    if case.more:
        path = os.path.join(tmp, "_reads_genome.0.bowtie")
        lines = open(path).read().split("\n")
        out = []
        for i in range(len(case.unit.pairs)):
            l1, l2 = lines[2 * i].split("\t"), lines[2 * i + 1].split("\t")
            assert int(l1[0]) == i and int(l2[0]) == i
            out += ["\t".join(l1), "\t".join(l2)]
            for left, other in case.more.get(i, ()):
                d1, d2 = left - case.unit.pairs[i].m1.pos, other - case.unit.pairs[i].m2.pos
                a, b = list(l1), list(l2)
                a[3], a[7] = str(int(l1[3]) + d1), str(int(l1[7]) + d2)
                b[3], b[7] = str(int(l2[3]) + d2), str(int(l2[7]) + d1)
                out += ["\t".join(a), "\t".join(b)]
        open(path, "w").write("\n".join(out) + "\n")
    if case.post:
        case.post(tmp)
    return tmp


class View:
    """What the predicates look at: the executor's front, the model over its hit records, each tile's arm and window width."""

    def __init__(self, case, front, tmp):
        self.case, self.f, self.tmp = case, front, tmp
        self.n_pos = int(front["n_pos"])
        self.m = FM.build(front["dhit"], self.n_pos, case.L, K, skip_x=left_x(case))
        self.arm, self.width = FM.arms(self.m)
        self.n = self.m["tile_cnt"][:self.m["n_tiles"]]
        self.n_tiles = self.m["n_tiles"]
        kept = self.m["kept"]
        self.kept = kept
        self.spans = set((self.m["t1"] - self.m["t0"] + 1)[kept].tolist())
        self.one_by_one = np.maximum(self.m["t1"] - self.m["t0"] - 3, 0)[kept]      # tiles of a hit that agx_k_hit_prep counts one by one
        self.place_of = np.empty(len(kept), np.int64)
        self.place_of[self.m["order"]] = np.arange(len(kept))
        self.file_ref = genome_of(tmp).encode()
        self.cm_n = front["cm_head"]["n"][:self.n_pos].astype(np.int64)

    def arms_present(self):
        return set(self.arm.tolist())

    def run_crosses_wave(self):
        """two neighbours of the device's order, on lanes 63 and 0 of consecutive wavefronts, kept and of one first tile"""
        o, ft, kept = self.m["order"], self.m["first_tile"], self.kept
        return any(kept[o[i]] and kept[o[i + 1]] and ft[o[i]] == ft[o[i + 1]] for i in range(63, len(o) - 1, 64))

    def skipped_inside_a_run(self):
        o, ft, kept = self.m["order"], self.m["first_tile"], self.kept
        return any(not kept[o[i]] and kept[o[i - 1]] and kept[o[i + 1]] and ft[o[i - 1]] == ft[o[i]] == ft[o[i + 1]] for i in range(1, len(o) - 1))

    def rank_differs_from_arrival(self, t):
        """tile t's list, ascending in file number, is not ascending in the hits' places of the device's order"""
        return bool(np.any(np.diff(self.place_of[FM.tile_list(self.m, t)]) < 0))

    def cm_runs(self):
        """lengths of the maximal stretches of positions that carry a conti-mer"""
        has = np.concatenate(([0], (self.cm_n > 0).astype(np.int64), [0]))
        edges = np.nonzero(np.diff(has))[0]
        return (edges[1::2] - edges[0::2]).tolist()

    def other_stretches(self):
        """(position, length, byte) of the maximal stretches of equal bytes of the unit sequence that are not A, C, G or T"""
        s, out, i = self.file_ref, [], 0
        while i < len(s):
            if s[i] in b"ACGT":
                i += 1
                continue
            j = i
            while j < len(s) and s[j] == s[i]:
                j += 1
            out.append((i, j - i, s[i]))
            i = j
        return out


def check_arms(case, view):
    for what, fn in case.arms:
        assert fn(view), "%s: does not reach its arm: %s" % (case.name, what)


# ---- hist: agx_k_hit_prep's histogram -------------------------------------------------------------------------------------------------------

def case_hist_spans():
    """Hits that reach 1, 2, 3 and 4 tiles at 2x100, both strands.  A read of 100 bases with k = 5 spans 96 positions, three tiles at most: four take a deletion (40M60D60M:
    156 positions), and such a hit is a long one (t1 - t0 = 3 = lookback)."""
    pairs = []
    for rev in (False, True):
        pairs += [P(64 * 10, cigar="64M36S", rev=rev)] * 2 + [P(64 * 14, rev=rev)] * 2 + [P(64 * 18 + 40, rev=rev)] * 2 + [P(64 * 22 + 40, cigar="40M60D60M", rev=rev)] * 2
    return Case("hist_spans", "hist", Unit(64 * 40, pairs), 100, [("hits of 1, 2, 3 and 4 tiles", lambda v: {1, 2, 3, 4} <= v.spans),
                                                                  ("the unit has no contig", lambda v: int(v.f["n_cm"]) == 0)])


def case_hist_span5():
    """2x150, 75M100D75M (246 positions) from lane 16: five tiles, the first one that agx_k_hit_prep counts one by one; from lane 0: four."""
    pairs = []
    for rev in (False, True):
        pairs += [P(64 * 10 + 16, 150, "75M100D75M", gap=600, rev=rev)] * 2 + [P(64 * 20, 150, "75M100D75M", gap=600, rev=rev)] * 2 + [P(64 * 6, 150, gap=600, rev=rev)]
    return Case("hist_span5", "hist", Unit(64 * 48, pairs), 150, [("a hit of five tiles", lambda v: 5 in v.spans), ("a hit of four", lambda v: 4 in v.spans),
                                                                  ("exactly one tile counted one by one", lambda v: 1 in v.one_by_one.tolist()),
                                                                  ("a window of four tiles", lambda v: v.m["lookback"] == 4)])


def case_hist_span7():
    """2x250, 125M160D125M (406 positions): seven tiles from lane 0, eight from lane 50 — the one-by-one loop runs three and four times."""
    pairs = []
    for rev in (False, True):
        pairs += [P(64 * 10, 250, "125M160D125M", gap=800, rev=rev)] * 2 + [P(64 * 24 + 50, 250, "125M160D125M", gap=800, rev=rev)] * 2 + [P(64 * 4, 250, gap=800, rev=rev)]
    return Case("hist_span7", "hist", Unit(64 * 60, pairs), 250, [("hits of seven and eight tiles", lambda v: {7, 8} <= v.spans),
                                                                  ("three and four tiles counted one by one", lambda v: {3, 4} <= set(v.one_by_one.tolist()))])


def case_hist_run65():
    """65 hits of one first tile at the head of the order: the run of equal tiles crosses the edge between the first two wavefronts."""
    pairs = [P(64 * 10 + i % 30, rev=(i % 3 == 0)) for i in range(65)]
    return Case("hist_run65", "hist", Unit(64 * 32, pairs), 100, [("a run of equal first tiles across a wavefront edge", lambda v: v.run_crosses_wave())])


def case_hist_count(n):
    """n hits in all: the last wavefront and the last block of agx_k_hit_prep full, one short, one over."""
    pairs = [P(256 + (i * 37) % 1500, rev=(i % 2 == 1)) for i in range(n)]
    return Case("hist_count_%d" % n, "hist", Unit(64 * 40, pairs), 100, [("%d hits" % n, lambda v: v.m["n_hits"] == n and int(v.kept.sum()) == n)])


def case_hist_dup():
    """Later hits of a pair: two that land within a read length of the pair's first hit and are dropped (AG:1650-1655) — skipped hits in the middle of a run of one first
    tile — and one further off that is kept."""
    pairs = [P(64 * 10 + i) for i in range(12)]
    more = {3: [(64 * 10 + 13, 64 * 10 + 413)], 5: [(64 * 20 + 5, 64 * 20 + 405)], 7: [(64 * 10 + 17, 64 * 10 + 417)], 9: [(64 * 10 + 2, 64 * 10 + 402)]}
    return Case("hist_dup", "hist", Unit(64 * 40, pairs), 100, [("three hits dropped, one later hit kept", lambda v: v.m["n_hits"] == 16 and int((~v.kept).sum()) == 3),
                                                               ("a skipped hit inside a run of one first tile", lambda v: v.skipped_inside_a_run())], more=more)


def case_hist_last_partial():
    """The last tile is partial and a hit's last arrival falls on the unit's last position."""
    G = 64 * 40 + 40
    x = G - 1 - (100 - K)
    pairs = [P(1000), P(1000, rev=True)] + [pair(x, x, "96M4S", "96M4S"), pair(x, x, "96M4S", "96M4S", rev=True)] * 2
    return Case("hist_last_partial", "hist", Unit(G, pairs), 100, [("a partial last tile", lambda v: v.n_pos % TILE != 0),
                                                                   ("a hit ends on the last position", lambda v: int(v.f["dhit"]["x_hi"][v.kept].max()) == v.n_pos - 1)])


# ---- window: the fast form of agx_k_tile_fill -------------------------------------------------------------------------------------------------

def case_window_64():
    """No long hit; tile 10's window holds exactly 64 hits and its list exactly 64 entries: the fast form's limit.  Tiles 0 and 1 (the window clipped at the front), an empty
    list between two full ones (20, 21, 22), an odd number of tiles with an entry in the last one (the wavefront's second tile does not exist)."""
    last = 64 * 40
    pairs = [P(5), P(70)] + [P(64 * 10)] * 64 + [P(64 * 20, cigar="64M36S")] * 3 + [P(64 * 22)] * 3 + [pair(last, last, "64M36S", "64M36S")] * 2
    return Case("window_64", "window", Unit(64 * 41, pairs), 100, [
        ("no long hit", lambda v: v.m["long_count"] == 0),
        ("a window of exactly 64 hits in the fast form", lambda v: v.width[10] == 64 and v.arm[10] == "fast"),
        ("a list of exactly 64 entries in the fast form", lambda v: v.n[10] == 64 and v.n[11] == 64 and v.arm[11] == "fast"),
        ("tiles 0 and 1 in the fast form", lambda v: v.arm[0] == "fast" and v.arm[1] == "fast"),
        ("an empty list between two full ones", lambda v: v.n[20] > 0 and v.n[21] == 0 and v.n[22] > 0),
        ("an odd tile count, the last tile's list not empty", lambda v: v.n_tiles % 2 == 1 and v.n[v.n_tiles - 1] > 0 and v.arm[v.n_tiles - 1] == "fast"),
        ("every list by the fast form", lambda v: v.arms_present() <= {"fast", "empty"})])


def case_window_65():
    """window_64's neighbour: 65 hits in tile 10's window — the general form, by window width alone."""
    pairs = [P(5), P(70)] + [P(64 * 10)] * 65 + [P(64 * 22)] * 3
    return Case("window_65", "window", Unit(64 * 40, pairs), 100, [
        ("no long hit", lambda v: v.m["long_count"] == 0),
        ("a window of 65 hits: the general form", lambda v: v.width[10] == 65 and v.arm[10] == "general_lds" and v.n[10] == 65),
        ("an even tile count", lambda v: v.n_tiles % 2 == 0),
        ("other tiles still fast", lambda v: v.arm[0] == "fast" and v.arm[22] == "fast")])


# ---- sort: the rank sorts at AGX_SORT_LDS -----------------------------------------------------------------------------------------------------

def case_sort(n, with_long):
    """Tile 10's list holds exactly n entries: n - 32 identical pairs that begin in it and 32 that begin in tile 9, their file numbers interleaved — the window delivers
    tile 9's hits first, so an entry's rank is not its arrival order.  512 sorts in LDS, 513 in global memory; without a long hit the general form is reached by the window's
    width, with one long hit elsewhere by that."""
    pairs, extras = [], 0
    for i in range(n - 32):
        pairs.append(P(64 * 10))
        if i % 15 == 7 and extras < 32:
            pairs.append(P(64 * 9 + 20))
            extras += 1
    assert extras == 32
    if with_long:
        pairs.append(P(64 * 30 + 40, cigar="40M60D60M"))
    arm = "general_lds" if n <= FM.SORT_LDS else "general_global"
    return Case("sort_%d_%s" % (n, "long" if with_long else "nolong"), "sort", Unit(64 * 48, pairs), 100, [
        ("%d long hits" % with_long, lambda v: v.m["long_count"] == int(with_long)),
        ("a list of %d entries through %s" % (n, arm), lambda v: v.n[10] == n and v.arm[10] == arm),
        ("rank differs from arrival order", lambda v: v.rank_differs_from_arrival(10))])


# ---- long: the list of long hits at AGX_LONG_MAX ------------------------------------------------------------------------------------------------

def case_long(n):
    """Exactly n long hits (40M60D60M, four tiles each).  1 and 1 024: the list of long hits, every tile through the general form; 1 025: one more than the list takes — the
    first attempt stops, the build repeats with the scatter fallback queued, and a 513-entry and a 512-entry list take both arms of agx_k_tile_sort."""
    pairs = [P(64 * (8 + i // 27) + 37 + i % 27, cigar="40M60D60M", rev=(i % 2 == 1)) for i in range(n)]      # (from lane 37 on, 156 positions reach a fourth tile)
    pairs += [P(64 * 100)] * 3
    arms = [("%d long hits" % n, lambda v: v.m["long_count"] == n)]
    device = {"dense_lists": 1, "long_count": n, "n_long": n}
    if n > FM.LONG_MAX:
        pairs += [P(64 * 105)] * 513 + [P(64 * 110)] * 512
        arms += [("a 513-entry and a 512-entry list in the dense form", lambda v: v.n[105] == 513 and v.arm[105] == "dense_global" and v.n[110] == 512 and v.arm[110] == "dense_lds")]
        device = {"dense_lists": 2, "long_count": n, "n_long": FM.LONG_MAX, "build_attempts": 2}
    else:
        arms += [("every list by the general form", lambda v: v.arms_present() <= {"general_lds", "empty"})]
        device["build_attempts"] = 1
    return Case("long_%d" % n, "long", Unit(64 * 120, pairs), 100, arms, device=device)


# ---- ref: agx_k_expand_ref / agx_k_patch_ref ----------------------------------------------------------------------------------------------------

def case_ref(extra):
    """n_pos = 4096 + extra (0, 1, 15 mod 16); stretches of N at position 0 (257 long: more than a block's 256 threads), of 256, 800 and 1, single IUPAC letters, and
    other bytes on the unit's last position: one N, a stretch of 20, one IUPAC letter."""
    G = 4096 + extra

    def post(tmp):
        s = list(genome_of(tmp))
        s[0:257] = "N" * 257
        s[1000:1256] = "N" * 256
        s[2000:2800] = "N" * 800
        s[3000] = "N"
        for j, i in enumerate((3100, 3101, 3103, 3500, 3564, 3999)):
            s[i] = IUPAC[(j + extra) % 10]
        if extra == 0:
            s[G - 1] = "N"
        elif extra == 1:
            s[G - 20:G] = "N" * 20
        else:
            s[G - 1] = "M"
        write_genome(tmp, "".join(s))

    pairs = [P(300), P(1300, rev=True), P(3050), P(3200, rev=True), P(3450)]

    def lens(v):
        return [(p, n) for p, n, _ in v.other_stretches()]
    return Case("ref_mod%d" % extra, "ref", Unit(G, pairs, seed=20 + extra), 100, [      # (a sequence of its own: no other unit leaves these bytes behind in a reused block)
        ("n_pos = %d mod 16" % extra, lambda v: v.n_pos == G and G % 16 == extra),
        ("a stretch of 257 at position 0", lambda v: (0, 257) in lens(v)),
        ("stretches of 256, 800 and 1", lambda v: {(1000, 256), (2000, 800), (3000, 1)} <= set(lens(v))),
        ("another byte on the last position", lambda v: any(p + n == G for p, n in lens(v))),
        ("single IUPAC letters", lambda v: sum(1 for _, n, b in v.other_stretches() if n == 1 and b != ord("N")) >= 5),
        ("few enough stretches for the packed form", lambda v: len(v.other_stretches()) <= v.n_pos // 256 + 1024)], post=post)


def case_ref_lower():
    """Lower case on every other position of half the unit: more stretches of other bytes than the packed form takes (n_pos / 256 + 1024) — the bytes cross as they are."""
    G = 8192

    def post(tmp):
        s = list(genome_of(tmp))
        for i in range(1000, 6000, 2):
            s[i] = s[i].lower()
        s[0], s[G - 1] = "n", "n"
        write_genome(tmp, "".join(s))
    pairs = [P(300), P(1300, rev=True), P(3050), P(6200, rev=True)]
    return Case("ref_lower", "ref", Unit(G, pairs, seed=40), 100, [("too many stretches for the packed form", lambda v: len(v.other_stretches()) > v.n_pos // 256 + 1024)],
                post=post, device={"ref_packed": 0})


# ---- codes: agx_k_expand_codes / agx_k_patch_codes ------------------------------------------------------------------------------------------------

def case_codes(L):
    """Reads of length L (57: rows of 60 bytes, 100: of 100 — no multiple of 16; 64: one) with N at read index 0, at L - 1, and both in the unit's last row."""
    gap = 300
    pairs = [P(300, L, gap=gap, bases={0: "N"}), P(500, L, gap=gap, rev=True, bases={L - 1: "N"}), P(700, L, gap=gap), P(705, L, gap=gap, rev=True, bases={L // 2: "N"}),
             P(900, L, gap=gap), P(64 * 30, L, gap=gap, bases={0: "N", L - 1: "N", L // 2: "N"})]

    def last_row_has_n(v):
        h = int(v.m["order"][-1])
        row = v.f["vcodes"][v.f["dhit"]["a_slot"][h]]
        return h == len(pairs) - 1 and row[0] == row[L - 1] and row[0] != row[1]
    return Case("codes_L%d" % L, "codes", Unit(64 * 40, pairs), L, [("the last hit of the order is the one with N at 0 and L - 1", last_row_has_n),
                                                                    ("read length %d" % L, lambda v: int(v.f["dhit"]["len"].max()) == L)])


def case_codes_few_hits():
    """Two hits: fewer than the three upload windows of the windowed form (windows without rows)."""
    pairs = [P(300, bases={99: "N"}), P(64 * 30, rev=True, bases={0: "N"})]
    return Case("codes_few_hits", "codes", Unit(64 * 40, pairs), 100, [("two hits", lambda v: v.m["n_hits"] == 2)])


def case_codes_tail():
    """Five hits of 57 bases, all in the first third of the unit: with three upload windows the first one reaches the last row (5 x 60 bytes: no multiple of 16), and that
    row ends in an N."""
    L = 57
    pairs = [P(64 * 2 + 7 * i, L, gap=300, rev=(i == 2), bases=({L - 1: "N"} if i == 4 else {})) for i in range(5)]
    return Case("codes_tail", "codes", Unit(64 * 60, pairs), L, [("every hit begins in the first of three windows", lambda v: int(v.m["t0"].max()) < v.n_tiles // 3),
                                                                 ("the rows' bytes are no multiple of 16", lambda v: (5 * ((L + 3) // 4 * 4)) % 16 != 0)])


# ---- rows: agx_k_expand_rows (AGX_ROW_DIFF=1) ---------------------------------------------------------------------------------------------------

def case_rows(n):
    """n rows — 63, 64, 65: around one block of 64 rows; 130: two blocks and a partial one — of every kind: equal to the reference, one base overridden, forty overridden
    (more differences than a row takes: explicit), a left mate with an insertion and a deletion (several runs), a soft-clipped one; both strands."""
    many = {j: "ACGT"[j % 4] for j in range(20, 60)}
    kinds = [dict(), dict(bases={10: "A"}), dict(bases={10: "C"}), dict(bases=many), dict(cigar="30M2I20M3D48M"), dict(cigar="30S70M"), dict(bases={0: "N", 50: "G"})]
    pairs = [P(200 + 23 * i, rev=(i % 2 == 1), **kinds[i % len(kinds)]) for i in range(n)]
    return Case("rows_%d" % n, "rows", Unit(64 * 64, pairs), 100, [("%d rows" % n, lambda v: v.m["n_hits"] == n and int(v.kept.sum()) == n),
                                                                  ("left mates of several runs", lambda v: int((v.f["dhit"]["a_nruns"] > 1).sum()) >= n // 8)], row_diff=True)


# ---- cm: agx_k_cm_layout / agx_k_cm_fill -------------------------------------------------------------------------------------------------------

CM_CHUNK = 2048


def case_cm_chunk():
    """Contigs of one PSL block whose conti-mers fill stretches of exactly AGX_CM_CHUNK - 1, AGX_CM_CHUNK and AGX_CM_CHUNK + 1 positions; the last one on the '-' strand."""
    contigs = [(500, 500 + CM_CHUNK - 1, "+"), (3000, 3000 + CM_CHUNK, "+"), (5500, 5500 + CM_CHUNK + 1, "-")]
    pairs = [P(600), P(3100, rev=True), P(7500)]
    return Case("cm_chunk", "cm", Unit(8192, pairs, contigs), 100, [("runs of 2 047, 2 048 and 2 049 conti-mers", lambda v: sorted(v.cm_runs()) == [CM_CHUNK - 1, CM_CHUNK, CM_CHUNK + 1])])


def case_cm_overlap():
    """Two overlapping contigs (a second conti-mer, rank 1, on a stretch of positions), one of them on the '-' strand, and a contig that ends on the unit's last position."""
    G = 8192
    contigs = [(2700, 3350, "+"), (3000, 3700, "-"), (900, 1400, "+"), (G - 600, G, "+")]
    pairs = [P(1000), P(2600), P(2900, rev=True), P(3300), P(G - 700, gap=500)]
    return Case("cm_overlap", "cm", Unit(G, pairs, contigs), 100, [("positions with two conti-mers", lambda v: int((v.cm_n == 2).sum()) >= 300),
                                                                   ("a conti-mer on the last position", lambda v: v.cm_n[v.n_pos - 1] >= 1),
                                                                   ("no position was appended", lambda v: v.n_pos == G)])


COUNTS = (1, 63, 64, 65, 255, 256, 257)


def cases():
    return ([case_hist_spans(), case_hist_span5(), case_hist_span7(), case_hist_run65()] + [case_hist_count(n) for n in COUNTS] + [case_hist_dup(), case_hist_last_partial(),
            case_window_64(), case_window_65(), case_sort(512, False), case_sort(513, False), case_sort(512, True), case_sort(513, True), case_long(1), case_long(1024), case_long(1025),
            case_ref(0), case_ref(1), case_ref(15), case_ref_lower(), case_codes(57), case_codes(64), case_codes(100), case_codes_few_hits(), case_codes_tail(),
            case_rows(63), case_rows(64), case_rows(65), case_rows(130), case_cm_chunk(), case_cm_overlap()])
