"""Hand-made units that pin passes 1, 2 and 3 of the node sweep (agx_k_node_sweep<1..3>, agx_kernels.hip), the device-side lists that hand a tile from one
pass to the next (mid_list, big_list, huge_list) and the node pool with its per-region slices and the spill area behind them (layout_regions, agx_engine.cpp).

The units are lean_units.Unit's, written by lean_units.write_unit (limit_1024 and limit_1025 are conftest.write_pileup_unit's): the CPU twin
(tests/test_sweep_cases.py) and the GPU file (tests/test_gpu_sweep_passes.py) build exactly the same inputs.  Every case names the arms it is there for as
predicates on a Ctx — the oracle's graph plus the tile-list lengths of the serial executor — and check_arms() asserts them, so a case cannot silently stop
reaching its arm.  The oracle decides what is correct; nothing here works out expected nodes or edges.

Which tiles each pass takes follows from the oracle's graph alone (sweep_model): a bucket only ever grows, so a pass gives up on a tile exactly when some
position of it ends with more variants than the pass's bucket holds.  The pool's first layout is restated from plan_capacities / spill_min / layout_regions
(pool_plan), a region's demand is the nodes of its 32 tiles (the region's counter goes on counting when its slice is full).

A pile-up of V variants on one tile: V pairs whose left mates share one alignment of 64 matches from lane 0 of the tile (64M36S: the arrivals are the tile's 64
positions and no other) while their other mates lie W + 1 apart.  A deep place bounded at one position comes from edge_units' helpers: reads that end (end_at)
or start (start_at) there, their mates edge_units.SEP apart, over a single-variant background (cover)."""
import numpy as np

import edge_units as EU
import lean_units as LU
from edge_units import OFF, SEP, cover, end_at, span, start_at
from lean_units import TILE, W, Unit, pair

# agx_kargs.h / agx_core.h
MID_WAVES, BIG_WAVES, HUGE_WAVES = 3072, 256, 32
MAXV_LDS, MAXV_MID, MAXV_BIG, MAXV_HUGE = 2, 4, 64, 1024
REGION_TILES = 32
PACKED_MAX = 65535          # entries of a tile list whose counters pass 0 can hold
NONE = 0xFFFFFFFF


# ---- the model ---------------------------------------------------------------------------------------------------------------------------

def per_pos(g):
    return np.diff(g["node_start"].astype(np.int64))


def per_tile(g, how):
    """how (np.max / np.sum) of the variants per position over each tile of 64 positions."""
    n_pos = int(g["n_pos"])
    n_tiles = (n_pos + TILE - 1) // TILE
    pad = np.zeros(n_tiles * TILE, np.int64)
    pad[:n_pos] = per_pos(g)
    return how(pad.reshape(n_tiles, TILE), axis=1)


def sweep_model(g, tile_len):
    """The tiles each pass takes: {"mid", "big", "huge"} -> ascending tile numbers."""
    tmax = per_tile(g, np.max)
    assert len(tile_len) == len(tmax)
    return {"mid": np.nonzero((tmax > MAXV_LDS) | (np.asarray(tile_len, np.int64) > PACKED_MAX))[0],
            "big": np.nonzero(tmax > MAXV_MID)[0], "huge": np.nonzero(tmax > MAXV_BIG)[0], "tmax": tmax}


def pool_plan(n_pos):
    """A first build's node pool (plan_capacities, spill_min, layout_regions without a measurement): (ids of every region's slice, ids of the spill area, regions)."""
    n_tiles = (n_pos + TILE - 1) // TILE
    regions = (n_tiles + REGION_TILES - 1) // REGION_TILES
    return (n_pos + n_pos // 4 + 4096) // regions, n_pos // 8 + 65536, regions


def region_demand(g):
    """Node ids every region of 32 tiles asks its counter for."""
    t = per_tile(g, np.sum)
    pad = np.zeros((len(t) + REGION_TILES - 1) // REGION_TILES * REGION_TILES, np.int64)
    pad[:len(t)] = t
    return pad.reshape(-1, REGION_TILES).sum(axis=1)


class Ctx:
    """What a case's arms are asserted on: the oracle's graph, the executor's tile-list lengths, and what follows from them."""

    def __init__(self, graph, tile_len=None):
        """tile_len None: a unit the executor refuses (no list of it is longer than pass 0's counters hold)."""
        self.n_pos = int(graph["n_pos"])
        if tile_len is None:
            tile_len = np.zeros((self.n_pos + TILE - 1) // TILE, np.int64)
        self.g, self.tile_len = graph, np.asarray(tile_len, np.int64)
        self.per = per_pos(graph)
        self.m = sweep_model(graph, self.tile_len)
        self.tmax = self.m["tmax"]
        self.share, self.spill, self.regions = pool_plan(self.n_pos)
        self.demand = region_demand(graph)

    def n(self, which):
        return len(self.m[which])

    def var_of_node(self):
        """Every node's variant index at its position."""
        ns = self.g["node_start"].astype(np.int64)
        return np.arange(int(self.g["n_nodes"])) - np.repeat(ns[:-1], self.per)

    def pos_of_node(self):
        return np.repeat(np.arange(self.n_pos), self.per)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, group, unit, arms, coverage=1, iv=LU.IV, windows=False, rebuild=False, pileup=None, overflow=False):
        """arms: [(description, fn(Ctx) -> bool)].  windows: the GPU file runs the case again under AGX_UPLOAD_WINDOWS=3; rebuild: and builds the resident unit a
        second time.  pileup: the unit is conftest.write_pileup_unit(run, pileup, spacing=130, genome_len=150000) instead of a lean_units.Unit.  overflow: the
        build must be refused with AGX_E_OVERFLOW."""
        self.name, self.group, self.unit, self.arms, self.coverage, self.iv = name, group, unit, arms, coverage, iv
        self.windows, self.rebuild, self.pileup, self.overflow = windows, rebuild, pileup, overflow

    def write(self, run):
        if self.pileup is not None:
            from conftest import write_pileup_unit
            return write_pileup_unit(run, self.pileup, spacing=130, genome_len=150000)
        return LU.write_unit(self.unit, run)


def check_arms(case, ctx):
    for what, fn in case.arms:
        assert fn(ctx), "%s: %s" % (case.name, what)


def pile(x, v, rev=False):
    """v variants at each of the 64 positions of the tile whose lane 0 is x, and nowhere else."""
    assert x % TILE == 0
    return [pair(x, x + 2000 + j * (W + 1), left_cigar="64M36S", other_cigar="100M", rev=rev) for j in range(v)]


def _stride(name, n_tiles, cycle, arms, first_tile=16):
    """n_tiles adjacent pile-ups whose variant counts cycle and whose strands alternate: the tile a wavefront sweeps second differs from its first in count and keys."""
    ps, counts = [], []
    for i in range(n_tiles):
        counts.append(cycle[i % len(cycle)])
        ps += pile((first_tile + i) * TILE, counts[-1], rev=bool(i & 1))
    G = ((first_tile + n_tiles) * TILE + 2000 + max(cycle) * (W + 1) + LU.L + 1023) // 1024 * 1024
    counts = np.array(counts, np.int64)

    def placed(c):      # every pile-up has its count on all 64 lanes of its own tile
        want = np.repeat(counts, TILE)
        return np.array_equal(c.per[first_tile * TILE:(first_tile + n_tiles) * TILE], want)
    return Case(name, "stride", Unit(G, ps), [("every tile holds its pile-up's count on all 64 lanes", placed)] + arms, rebuild=name != "stride_mid", windows=name == "stride_mid")


def _second_differs(which, waves):
    """Entry w + waves of a pass's list is swept by the wavefront that swept entry w.  The order of a list is the device's (the order in which the pass before
    gave up on the tiles), so which two tiles one wavefront meets is not in a test's hands: the arm says only that the list holds tiles of different counts,
    cycling from tile to tile, which makes a list on which every wavefront's second tile equals its first an order nobody has seen — not an impossible one."""
    return ("the %s list holds tiles of different counts (which of them one wavefront meets is the device's order)" % which,
            lambda c: len(set(c.tmax[c.m[which]].tolist())) >= 2)


def case_stride_mid():
    """Pass 1 makes a second iteration over mid_list; every seventh tile fails again in pass 1 (five variants) and goes on to pass 2: the `continue` behind a
    failed tile, the same wavefront going on with a dirty LDS bucket."""
    arms = [("more tiles on mid_list than pass 1 has wavefronts", lambda c: c.n("mid") > MID_WAVES),
            ("tiles that fail in pass 1", lambda c: c.n("big") >= 400),
            ("no tile beyond pass 2", lambda c: c.n("huge") == 0),
            ("tiles of exactly 3 and exactly 4 variants stay in pass 1", lambda c: {3, 4} <= set(c.tmax.tolist())),
            _second_differs("mid", MID_WAVES)]
    return _stride("stride_mid", MID_WAVES + 150, (3, 4, 3, 4, 3, 4, 5), arms)


def case_stride_big():
    """Pass 2 makes up to three iterations on global scratch (and the second half of agx_k_edge_sweep strides over big_list); the first build runs out of both
    the slices and the spill area: the `continue` behind a pool that ran out, then the regrow from the per-region demand."""
    arms = [("more than twice as many tiles on big_list as pass 2 has wavefronts", lambda c: c.n("big") > 2 * BIG_WAVES),
            ("every one of them came through mid_list", lambda c: c.n("mid") == c.n("big")),
            ("tiles of exactly 64 variants, none beyond", lambda c: c.n("huge") == 0 and int(c.tmax.max()) == MAXV_BIG),
            ("tiles of exactly 5 variants", lambda c: 5 in set(c.tmax.tolist())),
            ("the first layout's pool cannot hold the unit", lambda c: int(c.g["n_nodes"]) > c.share * c.regions + c.spill),
            _second_differs("big", BIG_WAVES)]
    return _stride("stride_big", 2 * BIG_WAVES + 5, (5, 40, 64, 9), arms)


def case_stride_huge():
    """Pass 3 makes up to three iterations over huge_list."""
    arms = [("more than twice as many tiles on huge_list as pass 3 has wavefronts", lambda c: c.n("huge") > 2 * HUGE_WAVES),
            ("tiles of exactly 65 variants", lambda c: 65 in set(c.tmax.tolist())),
            ("no position beyond pass 3's bucket", lambda c: int(c.tmax.max()) <= MAXV_HUGE),
            _second_differs("huge", HUGE_WAVES)]
    return _stride("stride_huge", 2 * HUGE_WAVES + 3, (65, 100, 70), arms)


# ---- limits ------------------------------------------------------------------------------------------------------------------------------

def deep_end(x, n):
    """n variants at x - 95 .. x, one from x + 1 on."""
    return cover(x - 300, x + 300) + [end_at(x, x + OFF + v * SEP) for v in range(1, n)]


def deep_start(x, n):
    """n variants at x .. x + 95, one in front of x."""
    return cover(x - 300, x + 300) + [start_at(x, x + OFF + v * SEP) for v in range(1, n)]


def _pass_arms(n):
    """Where a deepest position of exactly n variants sends its tile."""
    return [("the deepest position holds exactly %d variants" % n, lambda c: int(c.tmax.max()) == n),
            ("pass 0 %s the tile" % ("keeps" if n <= MAXV_LDS else "gives up on"), lambda c: (c.n("mid") > 0) == (n > MAXV_LDS)),
            ("pass 1 %s it" % ("keeps" if n <= MAXV_MID else "gives up on"), lambda c: (c.n("big") > 0) == (n > MAXV_MID)),
            ("pass 2 %s it" % ("keeps" if n <= MAXV_BIG else "gives up on"), lambda c: (c.n("huge") > 0) == (n > MAXV_BIG))]


LIMITS = (2, 3, 4, 5, 64, 65)
G_LIMIT = 32 * 1024         # (65 mates SEP apart behind a deep place need 14 000 positions)


def case_limit_lane(n, lane):
    """A deep place of exactly n variants whose edge is lane 0 (the place ends there: the tile holds it on lane 0 alone), lane 62 (it ends there: lane 63 holds one
    variant) or lane 63 (it starts there: the tile holds it on lane 63 alone)."""
    x = 40 * TILE + lane
    ps = deep_start(x, n) if lane == 63 else deep_end(x, n)
    t = x // TILE
    if lane == 0:
        on = [("lane 0 alone holds %d" % n, lambda c: c.per[x] == n and int(c.per[x + 1:(t + 1) * TILE].max()) == 1)]
    elif lane == 62:
        on = [("lanes 0 .. 62 hold %d, lane 63 one" % n, lambda c: (c.per[t * TILE:x + 1] == n).all() and c.per[x + 1] == 1)]
    else:
        on = [("lane 63 alone holds %d" % n, lambda c: c.per[x] == n and int(c.per[t * TILE:x].max()) == 1)]
    return Case("limit_%d_lane%d" % (n, lane), "limit", Unit(G_LIMIT, ps), _pass_arms(n) + on)


def case_limit_regions(n):
    """A deep place that ends on lane 0 of tile 32: all of tile 31, the last of the pool's first region, and the first position of the second region's first tile."""
    x = 32 * TILE
    on = [("tile 31 and lane 0 of tile 32 hold %d" % n, lambda c: (c.per[31 * TILE:x + 1] == n).all() and c.per[x + 1] == 1),
          ("two regions", lambda c: c.regions >= 2 and 31 // REGION_TILES != 32 // REGION_TILES)]
    return Case("limit_%d_regions" % n, "limit", Unit(G_LIMIT, deep_end(x, n)), _pass_arms(n) + on)


def case_limit_mod32(n):
    """A unit of 481 tiles: the pool's last region holds one tile, which the background reaches; a second deep place in tile 200, so that the deep tiles lie in
    two windows of an upload cut in three."""
    n_tiles = 15 * REGION_TILES + 1
    G = n_tiles * TILE
    x, y = 40 * TILE + 20, 200 * TILE + 20
    assert y + OFF + n * SEP + LU.L <= G
    ps = deep_end(x, n) + deep_start(y, n) + cover(G - 400, G - 100, 0)
    on = [("the last region holds one tile, with nodes", lambda c: c.n_pos == G and c.regions == 16 and c.demand[15] > 0),
          ("deep places of %d in tiles 40 and 200" % n, lambda c: c.per[x] == n and c.per[y] == n)]
    return Case("limit_%d_mod32" % n, "limit", Unit(G, ps), _pass_arms(n) + on, windows=n in (3, 65))


def case_limit_last(n):
    """The last position of a partial last tile holds n variants.  Only the last arrivals of reads whose last aligned index lands there reach it, and their
    other mates lie within a read length: insertVariation 0 (variants 26 apart) and an other mate with an insertion (edge_units.case_unit_end).  Two is the most: the
    loaders drop a mate whose insertion is long enough for a third variant (52 bases)."""
    G = 64 * 40 + 37
    last = G - 1
    ps = cover(1000, 1400) + cover(last - 300, last - 100, 0)
    ps += [pair(last - 95, last - 95, "96M4S", "96M4S"), pair(last - 96, last - 96, "97M3S", "97M3S")]
    ps += [pair(last - 95, last - 95, "96M4S", "%dM%dI5M" % (95 - 26 * v, 26 * v)) for v in range(1, n)]      # its index 95 pairs with the other mate's position last - 26 v
    on = [("the unit's last position, lane 36 of a partial tile, holds %d" % n, lambda c: c.n_pos == G and c.per[last] == n)]
    return Case("limit_%d_last" % n, "limit", Unit(G, ps), _pass_arms(n) + on, iv=0)


def _junction(x, n, n1):
    """n variants up to x, n1 from x + 1 on; the variants both sides hold step from x to x + 1."""
    out = [end_at(x, x + OFF + v * SEP) for v in range(n)]
    out += [span(x, x + OFF + v * SEP) for v in reversed(range(min(n, n1)))]
    out += [start_at(x + 1, x + 1 + OFF + v * SEP) for v in range(n1)]
    return out


NEIGHBOURS = [(a, b) for a in (3, 4) for b in (1, 2, 3, 4)] + [(a, b) for a in (1, 2) for b in (3, 4)]


def _bit15(c):
    """An edge from variant 3 of a position of 4 to variant 3 of the next position of 4, inside a tile: bit 15 of the sweep's edge matrix."""
    var, pos = c.var_of_node(), c.pos_of_node()
    es = c.g["edge_start"].astype(np.int64)
    src = np.repeat(np.arange(len(var)), np.diff(es))
    dst = c.g["edge_dst"].astype(np.int64)
    hit = (var[src] == 3) & (var[dst] == 3) & (pos[dst] == pos[src] + 1) & (pos[src] % TILE < 63) & (c.per[pos[src]] == 4) & (c.per[pos[dst]] == 4)
    return bool(hit.any())


def case_neighbours():
    """Pass-1 tiles in which positions of 3 and 4 variants stand next to positions of 1, 2, 3 and 4 (lanes 30 and 31): the write-out takes their x -> x + 1 edges from
    the edge matrix, variant 3 to variant 3 included."""
    ps = []
    at = {}
    for i, (a, b) in enumerate(NEIGHBOURS):
        x = 2048 + i * 1024 + 30
        at[(a, b)] = x
        ps += _junction(x, a, b)
    arms = [("%d next to %d on lanes 30 and 31" % ab, lambda c, ab=ab, x=x: (c.per[x], c.per[x + 1]) == ab) for ab, x in at.items()]
    arms += [("every deep tile stays in pass 1", lambda c: c.n("mid") >= len(NEIGHBOURS) and c.n("big") == 0),
             ("an edge from variant 3 to variant 3", _bit15)]
    return Case("neighbours", "limit", Unit(2048 + len(NEIGHBOURS) * 1024 + 2048, ps), arms, windows=True)


def _tied(c):
    """Nodes of variant index >= 2 whose two highest base votes are equal and not zero."""
    v = np.sort(c.g["node_cnt"][:, 1:].astype(np.int64), axis=1)
    return int(((c.var_of_node() >= 2) & (v[:, -1] == v[:, -2]) & (v[:, -1] > 0)).sum())


def case_ties():
    """Variants 2 and 3 of a pass-1 tile, and variants 2 .. 5 of a pass-2 tile, whose votes tie (two left mates of one variant that read different bases): the
    consensus rule A > C > G > T > N on an unpacked bucket."""
    def fn(x, n):
        out = cover(x - 300, x + 300)
        for v in range(1, n):
            a, b = "ACGTN"[v % 5], "ACGTN"[(v + 2) % 5]
            out += [start_at(x, x + OFF + v * SEP)]
            out[-1].bases = {20: a, 50: b}
            out += [start_at(x, x + OFF + v * SEP)]
            out[-1].bases = {20: b, 50: a}
        return out
    x4, x6 = 40 * TILE + 10, 80 * TILE + 10
    arms = [("four variants at one place, six at another", lambda c: c.per[x4 + 20] == 4 and c.per[x6 + 20] == 6),
            ("tied votes in variants of index >= 2", lambda c: _tied(c) >= 8)]
    return Case("ties", "limit", Unit(G_LIMIT, fn(x4, 4) + fn(x6, 6)), arms)


def _cov_at(c, n):
    var = c.var_of_node()
    return int(((var >= 2) & (c.g["node_key"][:, 0] == NONE) & (c.g["node_cnt"][:, 0] == n)).sum())


def case_coverage3():
    """At --coverage 3: non-contig variants of index >= 2 with coverage exactly 2 (dead: no side id) and exactly 3 (alive), in a pass-1 tile and in a pass-2 tile."""
    def fn(x, n):
        out = cover(x - 300, x + 300)
        for v in range(1, n):
            out += [start_at(x, x + OFF + v * SEP)] * (2 + v % 2)
        return out
    x4, x6 = 40 * TILE + 10, 80 * TILE + 10
    arms = [("four variants at one place, six at another", lambda c: c.per[x4 + 20] == 4 and c.per[x6 + 20] == 6),
            ("variants of index >= 2 with coverage exactly 2", lambda c: _cov_at(c, 2) > 0),
            ("variants of index >= 2 with coverage exactly 3", lambda c: _cov_at(c, 3) > 0)]
    return Case("coverage3", "limit", Unit(G_LIMIT, fn(x4, 4) + fn(x6, 6)), arms, coverage=3)


def case_limit_1024():
    """1024 variants at 96 positions, all 64 lanes of tile 16 among them: pass 3's bucket to the brim, and 63 x 1023 side ids in front of lane 63 of that tile."""
    arms = [("the deepest position holds exactly 1024 variants", lambda c: int(c.per.max()) == MAXV_HUGE),
            ("all 64 lanes of tile 16 hold 1024", lambda c: (c.per[16 * TILE:17 * TILE] == MAXV_HUGE).all()),
            ("96 such positions", lambda c: int((c.per == MAXV_HUGE).sum()) == 96)]
    return Case("limit_1024", "limit", None, arms, pileup=1024)


def case_limit_1025():
    """One variant more than pass 3's bucket holds: refused with AGX_E_OVERFLOW."""
    return Case("limit_1025", "limit", None, [("the deepest position holds 1025 variants", lambda c: int(c.per.max()) == MAXV_HUGE + 1)], pileup=1025, overflow=True)


# ---- the pool ----------------------------------------------------------------------------------------------------------------------------

SPILL_REGION = 96 // REGION_TILES


def case_spill():
    """A first build whose fourth region (tiles 96 .. 127, pile-ups of four variants on a thin background) asks for more ids than its slice holds and takes them from the spill area:
    node ids that are neither dense nor in position order, in one attempt."""
    ps = [pair(96 * 64 + i * 96, 96 * 64 + i * 96 + 3000 + j * (W + 1)) for i in range(21) for j in range(4)] + [pair(x, x + 400) for x in range(200, 60000, 50)]
    arms = [("the region's demand exceeds its slice", lambda c: c.demand[SPILL_REGION] > c.share),
            ("what is beyond the slice fits the spill area", lambda c: c.demand[SPILL_REGION] <= c.spill),
            ("no other region needs more than its slice", lambda c: all(d <= c.share for r, d in enumerate(c.demand.tolist()) if r != SPILL_REGION)),
            ("the region's tiles go beyond pass 0, none beyond pass 2", lambda c: c.n("mid") >= REGION_TILES and c.n("huge") == 0)]
    return Case("spill", "pool", Unit(65536, ps), arms, rebuild=True)


def cases():
    out = [case_stride_mid(), case_stride_big(), case_stride_huge()]
    for n in LIMITS:
        out += [case_limit_lane(n, 0), case_limit_lane(n, 62), case_limit_lane(n, 63), case_limit_regions(n), case_limit_mod32(n)]
    out += [case_limit_last(2), case_neighbours(), case_ties(), case_coverage3(), case_limit_1024(), case_limit_1025(), case_spill()]
    return out
