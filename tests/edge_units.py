"""Hand-made units that pin the edge build (agx_k_edge_sweep / agx_k_edge_jump / agx_k_edge_slow, agx_kernels.hip) path by path.

The units are lean_units.Unit's, written by lean_units.write_unit: the CPU twin (tests/test_edge_build_cases.py) and the GPU file
(tests/test_gpu_edge_build.py) build exactly the same inputs.  Each case names the edge-build paths it is there for as predicates on what the
serial executor reports (hostsim.sim.run(..., edges=True): counters of the paths, the slow list in the device's rule, pass J's steps and
inserts, the overflow appends); check_edges() asserts them, so a case cannot silently stop reaching its branch.  The oracle decides what is
correct; nothing here works out expected edges.

Node variants at a position come from mate positions further apart than lean_units.W (2 * insertVariation + 25): a read whose mate lies at
M at position X (its read index there pairs with the mate's same index) joins the variant of the other reads whose mates lie within W of M.
The helpers below place reads by that position: end_at / start_at / span / dele.
"""
import lean_units as LU
from lean_units import L, K, TILE, Unit, pair

OFF = 1000          # background reads: mate at X + OFF at position X
SEP = 200           # mate positions of different variants lie this far apart (> LU.W)


def end_at(x, m, rev=False):
    """A read whose last arrival (index L - K) is x, its mate at m there."""
    return pair(x - (L - K), m - (L - K), rev=rev)


def start_at(x, m, rev=False):
    """A read whose first arrival is x, its mate at m there."""
    return pair(x, m, rev=rev)


def span(x, m, q=40, rev=False):
    """A read whose index q arrives at x (and steps to x + 1), its mate at m there."""
    return pair(x - q, m - q, rev=rev)


def dele(x, ds, m=None, q=39):
    """A read whose index q arrives at x and then skips the lengths ds in turn (several deletions: one per entry, 20 matches apart)."""
    if m is None:
        m = x + OFF
    parts, used = ["%dM" % (q + 1)], q + 1
    for i, d in enumerate(ds):
        n = 20 if i + 1 < len(ds) else L - used
        parts.append("%dD%dM" % (d, n))
        used += n
    assert used == L
    return pair(x - q, m - q, left_cigar="".join(parts))


def cover(lo, hi, m_off=OFF):
    """Single-variant background: reads every 40 positions whose arrivals cover [lo, hi) with steps all the way."""
    return [pair(p, p + m_off) for p in range(lo - 40, hi, 40)]


def variants(x, n, at=end_at, m0=None):
    """n variants at x: n reads whose mates lie SEP apart there (variant v: mate at m0 + v * SEP)."""
    if m0 is None:
        m0 = x + OFF
    return [at(x, m0 + v * SEP) for v in range(n)]


class Case:
    def __init__(self, name, group, unit, want, coverage=1, windows=False, overflow=False, iv=LU.IV):
        """want: [(description, fn(out) -> bool)] on the executor's run(..., edges=True, graph=True) result.  windows: the case has edges across the
        window cuts of AGX_UPLOAD_WINDOWS = 2 and 3; overflow: the case appends to the overflow list; coverage, iv: the run's --coverage and
        insertVariation."""
        self.name, self.group, self.unit, self.want, self.coverage, self.windows, self.overflow, self.iv = name, group, unit, want, coverage, windows, overflow, iv


def check_edges(case, out):
    for what, fn in case.want:
        assert fn(out), "%s: %s" % (case.name, what)


# ---- predicates ------------------------------------------------------------------------------------------------------------------------

def ctr(name, at_least=1):
    return ("%s >= %d" % (name, at_least), lambda o: o["edges"][name] >= at_least)


def slow_where(desc, **want):
    """A slow position (device rule) whose SLOW_FIELDS match (a callable value is a predicate on the field)."""
    def fn(o):
        for s in o["slow"]:
            if all(v(int(s[k])) if callable(v) else int(s[k]) == v for k, v in want.items()):
                return True
        return False
    return ("slow position: " + desc, fn)


def lane(v):
    return lambda x: x % TILE == v


def pair_bit(vs, vd):
    return lambda p: (p >> (vs * 4 + vd)) & 1 == 1


def jstep_where(desc, fn1):
    return ("pass-J step: " + desc, lambda o: any(fn1(s) for s in o["jsteps"]))


def jins_where(desc, fn1):
    return ("pass-J insert: " + desc, lambda o: any(fn1(s) for s in o["jins"]))


def n_pos(o):
    return int(o["graph"]["n_pos"])


def _tile_max(o, t):
    ns = o["graph"]["node_start"].astype(int)
    lo, hi = t * TILE, min((t + 1) * TILE, n_pos(o))
    return int((ns[lo + 1:hi + 1] - ns[lo:hi]).max())


def cnt_at(o, x):
    ns = o["graph"]["node_start"]
    return int(ns[x + 1] - ns[x])


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

def _at(i, ln, gap=1024, first=2048):
    """Position of lane ln in region i."""
    return first + i * gap + ln


def case_boundary():
    """A. pass A's boundary blocks at lane 63: single -> single with a step, without one (one read ends on lane 63, the next starts on lane 0),
    with the step refused by agx_edge_allowed (the two positions' stored mate keys lie too far apart on one contig); single -> multi and multi -> single."""
    ps, contigs = [], []
    x = _at(0, 63); ps += cover(x - 200, x + 200)                                          # step
    x = _at(1, 63); ps += [end_at(x, x + OFF), start_at(x + 1, x + 1 + OFF)]               # no step
    ps += [end_at(x - 40, x - 40 + OFF), start_at(x + 41, x + 41 + OFF)]
    # refused: x's stored key comes from a read that ends there (mate at x + OFF), x + 1's from a read that skips x with a deletion (mate at x + OFF + 131);
    # a read stepping from x to x + 1 (mate 62 further) is compatible with both.  The mates lie on one contig, so the stored keys' contig offsets are
    # 131 > 2 * insertVariation + 25 apart: agx_edge_allowed refuses the step
    x = _at(2, 63); ps += [end_at(x, x + OFF), dele(x - 1, [1], x + OFF + 130, q=60), span(x, x + OFF + 62)] + cover(x + 42, x + 200, OFF + 131)
    contigs += [(x + OFF - 300, x + OFF + 500, "+")]
    x = _at(3, 63); ps += cover(x - 200, x + 1) + variants(x + 1, 2, start_at, x + 1 + OFF) + [span(x, x + OFF)]   # single -> multi
    x = _at(4, 63); ps += variants(x, 2, end_at) + [span(x, x + OFF)] + cover(x + 1, x + 200)                      # multi -> single
    want = [ctr("a_written"), ctr("a_nostep"), ctr("a_refused"),
            slow_where("single -> multi on lane 63", x=lane(63), who=1, n=1, n1=2, reg=1, pairs=lambda p: p != 0),
            slow_where("multi -> single on lane 63", x=lane(63), who=1, n=2, n1=1, reg=1, pairs=lambda p: p != 0)]
    return Case("boundary", "A", Unit(8 * 1024, ps, contigs), want)


def case_unit_end(m, extra, multi_last=False):
    """A. the unit ends at 64 m + extra; multi_last: the last position holds two variants (in a partial tile the device never runs pass A there,
    the executor's lane function does; at 64 m it is lane 63 without an x + 1: pass A lists it, pass B's context has no has1).

    Only the K2ONLY arrivals of reads whose last aligned index lands on the unit's last position reach it, and the left mate is the one further
    left at their common indices, so the other mates' positions there differ by less than a read length: at insertVariation 50 they are one
    variant.  The multi_last units run with insertVariation 0 (variants 25 apart) and an other mate with an insertion of 35 bases."""
    G = 64 * m + extra
    last = G - 1
    ps = cover(1000, 1400) + cover(last - 300, last - 100, 0)
    ps += [pair(last - 95, last - 95, "96M4S", "96M4S"), pair(last - 96, last - 96, "97M3S", "97M3S")]
    if multi_last:      # (its index 95 pairs with the other mate's position last - 35)
        ps += [pair(last - 95, last - 95, "96M4S", "60M35I5M")]
    name = "unit_end_%d%s" % (extra, "_multi" if multi_last else "")
    want = [("the last position holds %s" % ("two variants" if multi_last else "a node"), lambda o: cnt_at(o, n_pos(o) - 1) == (2 if multi_last else 1))]
    if multi_last and extra:
        want.append(("the partial tile's last position is not on the device's slow list", lambda o: n_pos(o) - 1 not in set(o["slow"]["x"].tolist())))
    if multi_last and not extra:
        want.append(slow_where("the unit's last position, lane 63, no x + 1", x=lambda x: x % TILE == 63, who=1, n=2, n1=0, reg=0))
    return Case(name, "A", Unit(G, ps), want, iv=0 if multi_last else LU.IV)


def case_grid(n_tiles):
    """A. a unit of n_tiles tiles covered end to end: pass A's boundary grid (n + 255) / 256 has a partial last block; every lane 63 carries an edge."""
    G = 64 * n_tiles
    ps = [pair(p, p) for p in range(0, G - L + 1, 60)] + [pair(G - L, G - L)]
    return Case("grid_%d" % n_tiles, "A", Unit(G, ps), [("every lane 63 but the last position's writes its edge", lambda o: o["edges"]["a_written"] == n_tiles - 1)])


def case_sweep_slow():
    """slow positions listed by the node sweep: a two-variant position in lanes 0..62 with a deletion step, in a pass-0 tile and in a pass-1 tile
    (a third variant elsewhere in the tile)."""
    ps = []
    x = _at(0, 30); ps += cover(x - 150, x + 150) + [span(x, x + OFF + SEP), dele(x, [5]), dele(x, [7], x + OFF + SEP)]
    x = _at(1, 30); ps += cover(x - 150, x + 150) + [span(x, x + OFF + SEP), dele(x, [5]), dele(x, [7], x + OFF + SEP)]
    ps += [span(x + 10, x + 10 + OFF + SEP), span(x + 10, x + 10 + OFF + 2 * SEP)]
    want = [slow_where("two variants, lanes 0..62, listed by the sweep", who=0, n=2, x=lambda x: x % TILE < 63),
            ("the same in a tile with three variants at a position (the device's pass 1)",
             lambda o: any(int(s["who"]) == 0 and int(s["n"]) >= 2 and _tile_max(o, int(s["x"]) // TILE) == 3 for s in o["slow"])),
            ctr("slow_sweep", 2)]
    return Case("sweep_slow", "S", Unit(8 * 1024, ps), want)


def case_jump():
    """J. one deletion; reads with two and with three deletions; a deletion into the next tile; a deletion whose target has two variants; one
    landing on the unit's last position."""
    ps = []
    x = _at(0, 20); ps += cover(x - 150, x + 200) + [dele(x, [6])]
    x = _at(1, 20); ps += cover(x - 150, x + 200) + [dele(x, [3, 4])]
    x = _at(2, 20); ps += cover(x - 150, x + 200) + [dele(x, [2, 3, 5])]
    x = _at(3, 60); ps += cover(x - 150, x + 200) + [dele(x, [9])]                          # target in the next tile
    x = _at(4, 20); ps += cover(x - 150, x + 200) + [dele(x, [8])] + [start_at(x + 9, x + 9 + OFF + SEP)]      # target with two variants
    G = 8 * 1024 + 37
    last = G - 1
    ps += cover(last - 300, last - 100, 0) + [pair(last - 95, last - 95, left_cigar="90M5D1M9S", other_cigar="90M5D1M9S")]      # index 90 lands on the last position
    want = [jstep_where("one deletion", lambda s: s["a_nruns"] == 2 and s["xs"] - s["x"] == 7),
            jstep_where("two deletions", lambda s: s["a_nruns"] == 3),
            jstep_where("three deletions", lambda s: s["a_nruns"] == 4),
            jstep_where("target in the next tile", lambda s: s["xs"] // TILE > s["x"] // TILE),
            jstep_where("target with two variants", lambda s: s["cnt_xs"] >= 2 and s["cnt_x"] == 1),
            ("a step onto the unit's last position", lambda o: any(int(s["xs"]) == n_pos(o) - 1 for s in o["jsteps"])),
            ctr("j_inserts", 8)]
    return Case("jump", "J", Unit(G, ps), want)


def case_jump_windows():
    """J. deletions whose source and target lie on either side of the window cuts n_tiles * w / W for W = 2 and 3 (agx_engine.cpp)."""
    G = 96 * TILE
    n_tiles = G // TILE
    ps = cover(200, G - 200, 0)
    cuts = sorted({n_tiles * w // W * TILE for W in (2, 3) for w in range(1, W)})
    for c in cuts:
        ps += [dele(c - 2, [4], c + 18), dele(c - 1, [11], c + 19)]
    want = [jins_where("across the cut at %d" % c, lambda s, c=c: s["x"] < c <= s["xs"]) for c in cuts]
    return Case("jump_windows", "J", Unit(G, ps), want, windows=True)


def case_register():
    """B. pass B's register path at lane 63: bucket pairs (1,2), (2,1), (2,3), (3,2), (4,4); pairs with vs != vd; contig keys that refuse some pairs;
    hits whose mate position carries two conti-mers (overlapping contigs): they leave the quick path inside a register context."""
    ps, contigs = [], []

    def junction(i, n, n1):
        """n variants at x (lane 63) and n1 at x + 1; reads step from x's variant v to x + 1's variant (listed in the opposite order: the steps
        are vs -> vd with vs != vd where both have a partner).  With n < n1, x + 1's first variant comes from a read that skips x with a
        deletion (first in x + 1's list): the steps then go to variants vd >= n."""
        x = _at(i, 63)
        out = [end_at(x, x + OFF + v * SEP) for v in range(n)]
        if n < n1:
            out += [dele(x - 1, [1], x + OFF + (n1 - 1) * SEP, q=60)]
        out += [span(x, x + OFF + v * SEP) for v in reversed(range(min(n, n1)))]
        out += [start_at(x + 1, x + 1 + OFF + v * SEP) for v in range(n1)]
        return out
    for i, (n, n1) in enumerate([(1, 2), (2, 1), (2, 3), (3, 2), (4, 4)]):
        ps += junction(i, n, n1)
    # refused pairs: the other mates of both variants lie on one contig, SEP apart: (0, 1) and (1, 0) fail agx_edge_allowed's mate clause
    x = _at(6, 63)
    ps += junction(6, 2, 2)
    contigs += [(x + OFF - 300, x + OFF + SEP + 300, "+")]
    # mates on two conti-mers
    x = _at(7, 63)
    ps += junction(7, 2, 2)
    contigs += [(x + OFF - 300, x + OFF + 100, "+"), (x + OFF - 100, x + OFF + 300, "-")]
    want = [slow_where("(%d,%d)" % nn, x=lane(63), n=nn[0], n1=nn[1], reg=1, pairs=lambda p: p != 0) for nn in [(1, 2), (2, 1), (2, 3), (3, 2), (4, 4)]]
    want += [slow_where("(%d,%d): a pair into a variant vd >= n" % nn, x=lane(63), n=nn[0], n1=nn[1], reg=1,
                        pairs=lambda p, n=nn[0]: any((p >> (vs * 4 + vd)) & 1 for vs in range(4) for vd in range(n, 4))) for nn in [(1, 2), (2, 3)]]
    want += [slow_where("a pair with vs != vd", reg=1, pairs=lambda p: any((p >> (vs * 4 + vd)) & 1 for vs in range(4) for vd in range(4) if vs != vd)),
             slow_where("a pair of a register context that the contigs refuse", reg=1, n=2, n1=2, allowed=lambda a: a & 0x33 != 0x33),
             slow_where("a hit whose mate carries two conti-mers leaves the quick path", reg=1, hit_ins=lambda n: n > 0),
             ctr("b_reg_pairs", 10)]
    return Case("register", "B", Unit(12 * 1024, ps, contigs), want)


def case_tile_list(n_entries):
    """B. a slow position (lane 63) whose tile list holds n_entries entries; the read that alone makes one of its pairs starts on lane 63, last in the list."""
    x = 2048 + 63
    base = variants(x + 1, 2, start_at, x + 1 + OFF) + cover(x - 300, x - 100)
    late = [start_at(x, x + OFF + SEP - 1)]
    probe = base + late
    fill = n_entries - _tile_entries(probe, x // TILE)
    ps = base + [span(x, x + OFF, q=50)] * fill + late
    want = [slow_where("tile list of %d entries" % n_entries, x=x, tile_len=n_entries, reg=1),
            slow_where("the last entry's pair (1, 1)", x=x, pairs=pair_bit(1, 1))]
    return Case("tile_list_%d" % n_entries, "B", Unit(6 * 1024, ps), want)


def _tile_entries(ps, t):
    """How many of the pairs' left mates touch tile t (what the tile's hit list holds; the cases keep every left mate = mate 1)."""
    n = 0
    for p in ps:
        lo = p.m1.pos
        hi = lo + sum(nn for nn, op in LU._cigar_ops(p.m1.cigar) if op in "MD") - K
        n += lo // TILE <= t <= hi // TILE
    return n


def case_general():
    """B. agx_edge_slow_hit for whole positions: a slow position with two conti-mers (overlapping contigs); a BIG-tile position with five variants."""
    ps, contigs = [], []
    x = _at(0, 63)
    ps += cover(x - 200, x + 1) + variants(x + 1, 2, start_at, x + 1 + OFF) + [span(x, x + OFF)]
    contigs += [(x - 300, x + 100, "+"), (x - 50, x + 300, "-")]
    x = _at(1, 20)
    ps += cover(x - 200, x + 200) + [span(x, x + OFF + v * SEP, q=30) for v in range(1, 5)] + [dele(x, [4], x + OFF + SEP)]
    want = [slow_where("two conti-mers at a small position", n=lambda n: n <= 4, n1=lambda n: 1 <= n <= 4, reg=0),
            slow_where("five variants (pass-2 tile)", n=5, reg=0), ctr("b_hit_inserts", 4)]
    return Case("general", "B", Unit(8 * 1024, ps, contigs), want)


def case_big_tiles():
    """BIG. single-variant positions inside a pass-2 tile and a pass-3 tile (more than 64 variants: a second build with pass 3 queued), lanes 62 and 63
    among them: pass A's wave loop writes their x -> x + 1 edges."""
    ps = []
    x = _at(0, 10); ps += cover(x - 200, x + 300) + [end_at(x, x + OFF + v * SEP) for v in range(1, 6)]
    x = _at(4, 10); ps += cover(x - 200, x + 300) + [end_at(x, x + OFF + v * SEP) for v in range(1, 70)]
    want = [ctr("a_written", 2 * 63 + 50), slow_where("five variants", n=6), slow_where("seventy variants", n=70)]
    return Case("big_tiles", "BIG", Unit(40 * 1024, ps), want)


def case_overflow():
    """OVF. sources with 4 distinct successors (x + 1 and three deletions), 5 and 9; four overflowing single-variant sources at consecutive positions of
    one tile (their flag bytes cover all four byte lanes of the word agx_slot_insert ORs into)."""
    ps = []
    x = _at(0, 20); ps += cover(x - 150, x + 200) + [dele(x, [d]) for d in (1, 2, 3)]
    x = _at(1, 20); ps += cover(x - 150, x + 200) + [dele(x, [d]) for d in (1, 2, 3, 4)]
    x = _at(2, 20); ps += cover(x - 150, x + 200) + [dele(x, [d]) for d in range(1, 9)]
    x = _at(3, 20); ps += cover(x - 150, x + 200) + [dele(x + j, [d]) for j in range(4) for d in range(1, 7)]
    want = [ctr("ovf_run_max", 4), ctr("ovf_distinct", 1 + 5 + 4 * 2),
            ("no duplicate appends", lambda o: o["edges"]["ovf_dup_appends"] == 0),
            ("a source with exactly four successors does not overflow", lambda o: not any(int(v["x"]) == _at(0, 20) for v in o["ovf"]))]
    return Case("overflow", "OVF", Unit(8 * 1024, ps), want, overflow=True)


def case_overflow_pruned():
    """OVF at --coverage 4: a single-variant source whose deletion targets 1..3 (the first three inserts: their slots) are pruned and whose targets
    4..8 (on the overflow list) survive.  Of its slots only x + 1 stays alive, so only the AGX_NF_EOVF flag keeps the walk from taking x as a
    forced run to x + 1.  (A target d is reached by the deletion reads of length <= d only: the background ends at x + 2.)"""
    x = _at(0, 20)
    ps = [end_at(x + 2, x + 2 + OFF)] * 4 + [end_at(x - 60, x - 60 + OFF)] * 4 + [dele(x, [d]) for d in range(1, 9)]
    want = [ctr("ovf_appends", 5), ("the source's slot targets are pruned, its overflow targets alive",
                                    lambda o: sorted(int(v["xs"]) - x for v in o["ovf"]) == list(range(5, 10)))]
    return Case("overflow_pruned", "OVF", Unit(6 * 1024, ps), want, coverage=4, overflow=True)


def case_overflow_dup():
    """OVF. a single-variant source on lane 63 whose x + 1 holds two variants and which deletes to eight more targets: pass J and pass B insert the same
    pairs, and a pair that overflows is listed twice."""
    x = _at(0, 63)
    ps = cover(x - 150, x + 1) + [span(x, x + OFF)] + [start_at(x + 1, x + 1 + OFF + SEP)] + cover(x + 1, x + 200) + [dele(x, [d]) for d in range(1, 9)]
    want = [ctr("ovf_dup_appends"), ctr("ovf_appends", 5), slow_where("the source on lane 63", x=lane(63), who=1, n=1, n1=2)]
    return Case("overflow_dup", "OVF", Unit(6 * 1024, ps), want, overflow=True)


def cases():
    return [case_boundary(), case_unit_end(40, 0), case_unit_end(40, 1), case_unit_end(40, 63),
            case_unit_end(40, 0, True), case_unit_end(40, 1, True), case_unit_end(40, 63, True),
            case_grid(255), case_grid(256), case_grid(257), case_grid(513),
            case_sweep_slow(), case_jump(), case_jump_windows(), case_register(), case_tile_list(64), case_tile_list(65), case_tile_list(130),
            case_general(), case_big_tiles(), case_overflow(), case_overflow_dup(), case_overflow_pruned()]
