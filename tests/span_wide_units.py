"""Hand-made units whose hit records fill the pair span's capped grid exactly, and a little more (tests/test_span_wide.py, tests/test_gpu_span_wide.py).

agx_k_span_mark and agx_k_sp_jumps (csrc/agx_span.hip) stride over all hit records from at most AGX_SPAN_BLOCKS workgroups of 256 lanes: below G = AGX_SPAN_BLOCKS * 256
records every lane sees one hit at most and nothing the loop carries from round to round is ever carried.  grid_hits() takes G from the library, CASES says how many
hit records each unit holds, and the tests assert the engine's n_hits against it, so a changed cap makes the cases fail instead of going stale.

The units are lean_units' (k = 5, insertVariation 50, coverage 1, L = 100) on a genome of N_POS positions: the pairs are drawn cyclically from N_SHAPES shapes — simple
mates on either strand and with either mate first in the file, a deletion in the left mate, an insertion in the other mate, a soft-clipped `a` mate whose `b` mate begins
left of it, fragments that end on the unit's last position (where the clamp to n_pos - 1 sits; a real unit cannot hold more: the build refuses an alignment beyond the unit
sequence), and pairs with a second, identical hit, which hit_prep marks AGX_HF_SKIP (AG:1650-1655) — the one way a loadable unit comes to a skipped hit record: mates on one
strand are the build's "BOWTIE ALIGNMENT ERROR".  So a unit's hit records are its pairs plus its second hits, and pairs_for() cuts the cycle where the records reach the count
asked for.

The device holds the hits in the order of their first tiles, hits of one tile in file order (agx_load.cpp), so the records behind G are those of the unit's highest first
tile: TOP_TILE is kept for five shapes of its own — simple, deletion, second hit, insertion, soft clip — that come round once per cycle, and every other shape begins left of
it.  device_order() says where each record of the file ends up; kinds_behind() is what the tests assert about the later rounds.

The text is made once, for the largest unit, with lean_units.write_unit; the smaller units are its first pairs (write_case)."""
import ctypes
import itertools
import os
import random
import re
import shutil

import numpy as np

import lean_units as LU
from lean_units import Mate, Pair, pair

N_POS = 40000
N_SHAPES = 2048
TILE = 64
TOP_TILE = (N_POS - 106) // TILE                     # the highest tile a left mate with a 5-base deletion can begin in (its alignment takes 105 positions)
K, IV, COVERAGE = LU.K, LU.IV, 1
SIMPLE, RUNS, SECOND = 0, 1, 2                       # what a hit record is: a fragment of two simple mates, a fragment with runs, the skipped second hit of a pair
CASES = {"G": lambda g: g,                           # one full round exactly; the loop's second test is base == n_hits
         "G+1": lambda g: g + 1,                     # the second round holds one hit: block 0, lane 0
         "G+257": lambda g: g + 257,                 # the second round fills block 0 and holds one hit in block 1
         "2G+65": lambda g: 2 * g + 65}              # a third round that begins in a wavefront's second lane group


def grid_hits():
    """G: the hit records one round of the mark pass takes, from the library (agx_span_partials: four partials per workgroup), else from AGX_SPAN_BLOCKS in agx_kargs.h."""
    import aligngraph_amd as A
    try:
        f = ctypes.CDLL(A.LIB_PATH).agx_span_partials
        f.argtypes, f.restype = [ctypes.c_uint32], ctypes.c_uint32
        return int(f(0xFFFFFFFF)) // 4 * 256
    except (OSError, AttributeError):
        with open(os.path.join(os.path.dirname(A.LIB_PATH), "csrc", "agx_kargs.h")) as h:
            return int(re.search(r"#define\s+AGX_SPAN_BLOCKS\s+(\d+)u?", h.read()).group(1)) * 256


class Shape:
    def __init__(self, what, p, second=False):
        """what: SIMPLE or RUNS; p: the lean_units.Pair; second: the pair has a second, identical hit"""
        self.what, self.pair, self.second = what, p, second
        r = [_aligned(m) for m in (p.m1, p.m2)]
        self.f_lo, self.f_hi = min(a for a, _ in r), min(max(b for _, b in r), N_POS - 1)      # the fragment, from the positions and CIGARs as written


def _aligned(m):
    """(first, last) aligned reference position of a mate: POS, and POS plus what its M and D operations take"""
    return m.pos, m.pos + sum(n for n, op in LU._cigar_ops(m.cigar) if op in "MD") - 1


def shapes():
    """The N_SHAPES shapes of a cycle.  Every shape's left mate begins left of TOP_TILE but for the last five."""
    rnd = random.Random(7)
    out = []
    top = TOP_TILE * TILE
    for s in range(N_SHAPES - 5):
        left, off, kind = rnd.randrange(0, top - 30), rnd.randrange(0, 500), s % 8
        other = min(left + max(off, 5 if kind in (2, 3) else 0), N_POS - 105)      # (an indel's pair keeps its left mate left at every read index: off >= 5)
        if kind == 0:
            out.append(Shape(SIMPLE, pair(left, other)))
        elif kind == 1:
            out.append(Shape(SIMPLE, pair(left, other, rev=True)))
        elif kind == 2:
            out.append(Shape(RUNS, pair(left, other, left_cigar="40M5D60M")))
        elif kind == 3:
            out.append(Shape(RUNS, pair(left, other, other_cigar="50M3I47M", rev=True)))
        elif kind == 4:      # the soft-clipped mate is `a` (read index 0 of it lies left of the other mate's) and begins 20 to 30 positions right of its `b` mate
            out.append(Shape(RUNS, Pair(Mate(left + 30 - off % 11, "30S70M", False), Mate(left, "%dM" % LU.L, True))))
        elif kind == 5:
            out.append(Shape(SIMPLE, pair(left, other), second=True))
        elif kind == 6:      # ends on the unit's last position
            left = min(left, N_POS - 100 - off)
            out.append(Shape(SIMPLE, pair(left, N_POS - 100, rev=bool(s & 8))))
        else:
            out.append(Shape(SIMPLE, pair(left, other, left_is_mate2=True)))
    t = [top + 3, top + 9, top + 14, top + 18, top - 8]
    out += [Shape(SIMPLE, pair(t[0], N_POS - 100)),
            Shape(SIMPLE, pair(t[1], t[1] + 10), second=True),
            Shape(RUNS, pair(t[2], N_POS - 97, other_cigar="50M3I47M")),
            Shape(RUNS, Pair(Mate(t[4] + 30, "30S70M", True), Mate(t[4], "%dM" % LU.L, False))),
            Shape(RUNS, pair(t[3], N_POS - 100, left_cigar="40M5D60M", rev=True))]
    assert len(out) == N_SHAPES
    return out


def pairs_for(n_hits, sh):
    """(number of pairs, second: a bool per pair) of the unit with exactly n_hits hit records: the cycle of shapes cut where the records reach n_hits; the last pair goes
    without its second hit where that would be one record too many."""
    second = np.array([s.second for s in sh], bool)
    per_cycle = N_SHAPES + int(second.sum())
    sec = np.tile(second, n_hits // per_cycle + 1)
    upto = np.cumsum(1 + sec.astype(np.int64))
    n = int(np.searchsorted(upto, n_hits, side="left")) + 1
    sec = sec[:n].copy()
    if upto[n - 1] > n_hits:
        sec[n - 1] = False
    assert n + int(sec.sum()) == n_hits
    return n, sec


def records(n_hits, sh):
    """The unit's hit records in FILE order, from the construction: what (SIMPLE / RUNS / SECOND), f_lo, f_hi (of a SECOND record: its first hit's, not a fragment),
    first_x — the first aligned position of the hit's left mate, whose tile the device orders by."""
    n, sec = pairs_for(n_hits, sh)
    shape = np.arange(n) % N_SHAPES
    rec_pair = np.repeat(np.arange(n), 1 + sec.astype(np.int64))
    is_second = np.concatenate(([False], rec_pair[1:] == rec_pair[:-1]))
    s = shape[rec_pair]
    what = np.where(is_second, SECOND, np.array([x.what for x in sh])[s])
    left_first = np.array([min(m.pos for m in (x.pair.m1, x.pair.m2)) if x.pair.m1.cigar[:3] != "30S" else x.pair.m1.pos for x in sh])
    return {"what": what, "f_lo": np.array([x.f_lo for x in sh], np.int64)[s], "f_hi": np.array([x.f_hi for x in sh], np.int64)[s], "first_x": left_first[s], "n_pairs": n}


def device_order(first_x):
    """perm: the file number of the record at each place of the device's order — ascending first tile, the hits of one tile in file order."""
    return np.argsort(np.asarray(first_x) // TILE, kind="stable")


def kinds_behind(what_in_device_order, g):
    """How many SIMPLE, RUNS and SECOND records lie at index >= g."""
    tail = np.asarray(what_in_device_order)[g:]
    return {k: int((tail == k).sum()) for k in (SIMPLE, RUNS, SECOND)}


def assert_later_rounds(name, what_in_device_order, g):
    """A case must not silently stop putting the interesting kinds into the later rounds.  G: nothing lies behind G.  G + 1: the one record of the second round is a
    fragment (a skipped hit there would make the round's loss invisible).  Above: a skipped hit, a fragment with runs and a simple fragment each lie behind G."""
    n = kinds_behind(what_in_device_order, g)
    behind = len(what_in_device_order) - g
    assert sum(n.values()) == behind == CASES[name](g) - g, (name, n, behind)
    if behind == 1:
        assert n[SECOND] == 0, (name, "the one record behind G is a skipped hit", n)
    elif behind > 1:
        assert n[SIMPLE] >= 1 and n[RUNS] >= 1 and n[SECOND] >= 1, (name, "a kind of record is missing behind G: simple, with runs, skipped", n)
    return n


def write_full(run, g, sh):
    """The text of the largest unit's pairs, each written once (no second hits): run/tmp."""
    n = max(pairs_for(f(g), sh)[0] for f in CASES.values())
    return LU.write_unit(LU.Unit(N_POS, [sh[i % N_SHAPES].pair for i in range(n)]), run)


def write_case(full_tmp, run, n_hits, sh):
    """The unit of n_hits hit records in run/tmp: the first pairs of the full text, the SAM lines of a pair with a second hit written twice.  Returns tmp."""
    n, sec = pairs_for(n_hits, sh)
    tmp = os.path.join(run, "tmp")
    os.makedirs(tmp, exist_ok=True)
    for name in ("_genome.0.fa", "_contigs.fa", "_contigs_genome.0.psl"):
        shutil.copyfile(os.path.join(full_tmp, name), os.path.join(tmp, name))
    with open(os.path.join(full_tmp, "_reads.fa")) as src, open(os.path.join(tmp, "_reads.fa"), "w") as dst:
        dst.writelines(itertools.islice(src, 4 * n))
    with open(os.path.join(full_tmp, "_reads_genome.0.bowtie")) as src, open(os.path.join(tmp, "_reads_genome.0.bowtie"), "w") as dst:
        for i, twice in enumerate(sec.tolist()):
            two = src.readline() + src.readline()
            dst.write(two + two if twice else two)
    return tmp
