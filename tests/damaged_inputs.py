"""One table of damages to the two binary doors into the engine: tmp/_agx_pairs.<u>.bin (staged read alignments) and tmp/_agx_unit.<u>.bin (the unit cache).

Both files are refused by CONTENT, not only by length (aligngraph_amd/csrc/agx_host.h "content rules"; DESIGN.md "Rejected inputs").  Every entry of TABLE changes one
field of an otherwise intact file — a section, an element, a field, a value — and says what must become of it: `accepted`, or the NAME of the rule that refuses it.  Where
a rule has a boundary the table holds both sides: the first refused value and the last accepted one.  An accepted value is chosen so that the file stays coherent (another
rule would otherwise refuse it for a reason of its own); where that cannot be, the entry names the rule that does refuse it and says why.

The doors (all CPU; nothing here touches a device):
  pairs         the staged-pairs file itself: a copy of its bytes, damaged, written out and opened the way the engine opens it (hostsim: agx_hostsim_check_pairs_file)
  cache         the arrays of a unit cache made of the unit's text in memory, read alignments through the general loader (rows = read slots)
  cache_fast    the same through the fast loader (rows = offsets into tmp/_reads.fa)
  cache_header  the header save_cache would write for the `cache` arrays
The record types mirror agx_whit, agx_wside, agx_wrun and agx_cmseg (agx_core.h) and the two headers (agx_host.h); their sizes are asserted against the sizes[] the
headers carry."""
import ctypes
import os

import numpy as np

from hostsim import sim

WHIT = np.dtype([("a", "<u4"), ("b", "<u4"), ("row", "<u4"), ("len", "<u2"), ("flags", "u1"), ("back", "u1")])
WSIDE = np.dtype([("runs1", "<u4"), ("runs2", "<u4"), ("nruns", "<u4")])
WRUN = np.dtype([("t", "<u4"), ("q", "<u2"), ("n", "<u2")])
CMSEG = np.dtype([(f, "<u4") for f in ("pos0", "len", "cid", "coff0", "dcoff", "rank", "hop_str0", "hop_len0", "hop_end", "elem0")])
REV1, REV2, LEFT2, RUNS1, RUNS2, DUP = 1, 2, 4, 8, 16, 32
P_SECTIONS = ("hits", "sides", "runs", "codes", "other", "otherb", "jump")                      # pairsfile::S_*
C_SECTIONS = ("hits", "runs", "codes", "segs", "chain_end", "rows", "ref", "cm_cnt", "chain_str", "initial", "bases", "other", "sides", "jump", "otherb")      # cachefile::S_*
PAIRS_HEADER = np.dtype([("magic", "u1", 8), ("version", "<u4"), ("k", "<u4"), ("batch", "<u4"), ("stride", "<u4"), ("maxlen", "<u4"), ("n_rows", "<u4"),
                         ("nh", "<u8"), ("n_sides", "<u8"), ("n_runs", "<u8"), ("n_codes", "<u8"), ("n_other", "<u8"), ("n_jump", "<u8"), ("pairs_in_file", "<u8"), ("sam_pairs", "<u8"),
                         ("sizes", "<u4", 3), ("off", "<u8", len(P_SECTIONS)), ("len", "<u8", len(P_SECTIONS))], align=True)
CACHE_HEADER = np.dtype([("magic", "u1", 8), ("version", "<u4"), ("batch", "<u4"), ("stamp", "<u8", (6, 2)),
                         ("n_pos", "<u8"), ("n_ref", "<u8"), ("nh", "<u8"), ("n_runs", "<u8"), ("n_cm", "<u8"), ("n_segs", "<u8"), ("n_seg0", "<u8"), ("n_rows", "<u8"), ("n_chain_end", "<u8"),
                         ("n_codes", "<u8"), ("pairs_in_file", "<u8"), ("sam_pairs", "<u8"),
                         ("stride", "<u4"), ("maxlen", "<u4"), ("n_slots", "<u4"), ("k", "<u4"), ("rows_in_reads", "<u4"), ("slot_stride", "<u4"), ("n_sides", "<u8"), ("n_jump", "<u8"),
                         ("sizes", "<u4", 5), ("off", "<u8", len(C_SECTIONS)), ("len", "<u8", len(C_SECTIONS))], align=True)
SECTION_TYPES = {"hits": WHIT, "sides": WSIDE, "runs": WRUN, "jump": np.dtype("<u4"), "other": np.dtype("<u8"), "otherb": np.dtype("u1"), "codes": np.dtype("u1"),
                 "segs": CMSEG, "cm_cnt": np.dtype("u1"), "chain_end": np.dtype("<u4")}
ACCEPTED = "accepted"


def _lib():
    L = sim._lib_now()
    if not getattr(L, "_damaged_ready", False):
        L.agx_hostsim_rule_names.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        L.agx_hostsim_check_pairs_file.argtypes = [ctypes.c_char_p, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        L.agx_hostsim_cache_arrays.restype = ctypes.c_void_p
        L.agx_hostsim_cache_arrays.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.POINTER(SimCache), ctypes.c_char_p, ctypes.c_size_t]
        L.agx_hostsim_cache_free.argtypes = [ctypes.c_void_p]
        L.agx_hostsim_cache_check.argtypes = [ctypes.POINTER(SimCache), ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        L.agx_hostsim_cache_header_check.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
        L._damaged_ready = True
    return L


def rule_names():
    """Every name the content checks can return (agx_load.cpp: RULE_NAMES)."""
    buf = ctypes.create_string_buffer(8192)
    n = _lib().agx_hostsim_rule_names(buf, 8192)
    names = buf.value.decode().split()
    assert n == len(names) and len(set(names)) == n
    return names


class SimCache(ctypes.Structure):      # agx_sim_cache (tests/hostsim/agx_hostsim.cpp)
    _fields_ = [(n, ctypes.c_void_p) for n in ("hits", "sides", "runs", "jump", "other", "segs", "cm_cnt", "chain_end", "rows", "header")] + \
               [(n, ctypes.c_ulonglong) for n in ("nh", "n_sides", "n_runs", "n_jump", "n_other", "n_segs", "n_pos", "n_chain_end", "n_rows", "n_cm", "chain_str_len", "reads_size", "file_size")] + \
               [(n, ctypes.c_uint32) for n in ("stride", "maxlen", "n_slots", "rows_in_reads", "header_bytes", "pad")]


def _view(ptr, dtype, count):
    if not count or not ptr:
        return np.zeros(0, dtype)
    return np.frombuffer((ctypes.c_char * (count * dtype.itemsize)).from_address(ptr), dtype, count)


class Door:
    """An intact input with its sections as writable numpy arrays (self.a), its header (self.h, one record) where it has one, and its counts (self.n).  verdict(): what the
    checks say to its present state; restore(): intact again."""
    def is_jump(self, i):
        """pass J's list names hit i: its left mate has two runs or more"""
        w = self.a["hits"][i]
        bit = RUNS2 if w["flags"] & LEFT2 else RUNS1
        if not w["flags"] & bit:
            return False
        sd = self.a["sides"][int(w["a"] if w["flags"] & RUNS1 else w["b"])]
        return int(sd["nruns"] >> 16 if w["flags"] & LEFT2 else sd["nruns"] & 0xFFFF) >= 2

    def side_of(self, i):
        w = self.a["hits"][i]
        return int(w["a"] if w["flags"] & RUNS1 else w["b"])

    def mate_runs(self, i, mate):
        """(first, count) of the runs of mate 1 or 2 of hit i; count 0: the mate is one full-length run"""
        w = self.a["hits"][i]
        if not w["flags"] & (RUNS1 if mate == 1 else RUNS2):
            return 0, 0
        sd = self.a["sides"][self.side_of(i)]
        return (int(sd["runs1"]), int(sd["nruns"] & 0xFFFF)) if mate == 1 else (int(sd["runs2"]), int(sd["nruns"] >> 16))

    def first_hit(self, pred):
        for i in range(len(self.a["hits"])):
            if pred(i, self.a["hits"][i]):
                return i
        raise LookupError("the unit has no such hit")


class PairsDoor(Door):
    kind = "pairs"

    def __init__(self, path, n_pos, scratch, k=0, batch=0, threads=2):
        self.bytes0 = open(path, "rb").read()
        self.n_pos, self.scratch, self.k, self.batch, self.threads = n_pos, scratch, k, batch, threads
        self.restore()
        h = self.h
        assert PAIRS_HEADER.itemsize == 224 and tuple(h["sizes"]) == (WHIT.itemsize, WSIDE.itemsize, WRUN.itemsize)

    def restore(self):
        self.buf = bytearray(self.bytes0) + bytearray(1 << 16)      # (slack: an entry may make the file longer)
        self.file_size = len(self.bytes0)
        self.h = np.frombuffer(self.buf, PAIRS_HEADER, 1)[0]
        h = self.h
        self.a = {}
        for i, s in enumerate(P_SECTIONS):
            dt = SECTION_TYPES[s]
            self.a[s] = np.frombuffer(self.buf, dt, int(h["len"][i]) // dt.itemsize, int(h["off"][i]))
        self.n = dict(nh=int(h["nh"]), n_sides=int(h["n_sides"]), n_runs=int(h["n_runs"]), n_jump=int(h["n_jump"]), n_other=int(h["n_other"]), n_rows=int(h["n_rows"]),
                      stride=int(h["stride"]), maxlen=int(h["maxlen"]), n_pos=self.n_pos)

    def set_count(self, name, value):
        """a count with the length of its section, so that the header stays consistent"""
        sec = {"n_jump": "jump", "n_sides": "sides", "n_other": "other", "nh": "hits", "n_runs": "runs"}[name]
        self.h[name] = value
        self.h["len"][P_SECTIONS.index(sec)] = value * SECTION_TYPES[sec].itemsize

    def write(self, path):
        with open(path, "wb") as f:
            f.write(bytes(self.buf[:self.file_size]))

    def verdict(self):
        path = os.path.join(self.scratch, "_damaged_pairs.bin")
        self.write(path)
        rule = ctypes.create_string_buffer(256)
        rc = _lib().agx_hostsim_check_pairs_file(path.encode(), self.n_pos, self.k, self.batch, self.threads, rule, 256)
        assert rc in (0, 1, 2), (rc, rule.value)
        return ACCEPTED if rc == 0 else rule.value.decode()


class CacheDoor(Door):
    def __init__(self, tmp_dir, unit, k, batch=1000000, fast=False, threads=2, header=False):
        self.kind = "cache_header" if header else "cache_fast" if fast else "cache"
        self.c = SimCache()
        msg = ctypes.create_string_buffer(512)
        self.handle = _lib().agx_hostsim_cache_arrays(str(tmp_dir).encode(), unit, k, batch, threads, int(fast), ctypes.byref(self.c), msg, 512)
        if not self.handle:
            raise sim.SimError(-1, msg.value.decode())
        self.k, self.batch, self.threads, self.header = k, batch, threads, header
        c = self.c
        self.a = {"hits": _view(c.hits, WHIT, c.nh), "sides": _view(c.sides, WSIDE, c.n_sides), "runs": _view(c.runs, WRUN, c.n_runs), "jump": _view(c.jump, np.dtype("<u4"), c.n_jump + 1),
                  "other": _view(c.other, np.dtype("<u8"), c.n_other), "segs": _view(c.segs, CMSEG, c.n_segs), "cm_cnt": _view(c.cm_cnt, np.dtype("u1"), c.n_pos),
                  "chain_end": _view(c.chain_end, np.dtype("<u4"), c.n_chain_end), "rows": _view(c.rows, np.dtype("<u8" if fast else "<u4"), c.n_rows)}
        assert c.header_bytes == CACHE_HEADER.itemsize == 512
        self.hv = _view(c.header, CACHE_HEADER, 1)
        self.h = self.hv[0]
        assert tuple(self.h["sizes"]) == (WHIT.itemsize, WRUN.itemsize, CMSEG.itemsize, CACHE_HEADER.itemsize, WSIDE.itemsize)
        self.keep = {s: v.copy() for s, v in self.a.items()}
        self.keep_h = self.h.copy()
        self.keep_c = bytes(memoryview(self.c))
        self.restore()

    def restore(self):
        for s, v in self.a.items():
            v[...] = self.keep[s]
        self.hv[0] = self.keep_h
        ctypes.memmove(ctypes.byref(self.c), self.keep_c, ctypes.sizeof(self.c))
        c = self.c
        self.file_size = int(c.file_size)
        self.n = dict(nh=int(c.nh), n_sides=int(c.n_sides), n_runs=int(c.n_runs), n_jump=int(c.n_jump), n_other=int(c.n_other), n_rows=int(c.n_rows), stride=int(c.stride), maxlen=int(c.maxlen),
                      n_pos=int(c.n_pos), n_segs=int(c.n_segs), n_chain_end=int(c.n_chain_end), chain_str_len=int(c.chain_str_len), reads_size=int(c.reads_size), n_slots=int(c.n_slots), n_cm=int(c.n_cm))

    def set_count(self, name, value):
        setattr(self.c, name, value)

    def verdict(self):
        rule = ctypes.create_string_buffer(256)
        if self.header:
            rc = _lib().agx_hostsim_cache_header_check(self.c.header, self.file_size, self.batch, self.k, rule, 256)
        else:
            rc = _lib().agx_hostsim_cache_check(ctypes.byref(self.c), self.threads, rule, 256)
        assert rc in (0, 1, 2), (rc, rule.value)
        return ACCEPTED if rc == 0 else rule.value.decode()

    def close(self):
        if self.handle:
            self.a = self.keep = None
            self.h = self.hv = None
            _lib().agx_hostsim_cache_free(self.handle)
            self.handle = None


class CacheFileDoor(Door):
    """A cache file as the engine wrote it (tests/test_gpu_damaged_inputs.py): its bytes, damaged by a table entry and written back.  No verdict here: the engine gives it."""
    def __init__(self, path, reads_size=0):
        self.path, self.bytes0 = path, open(path, "rb").read()
        self.reads_size = reads_size
        self.restore()
        assert CACHE_HEADER.itemsize == int(self.h["sizes"][3])

    def restore(self):
        self.buf = bytearray(self.bytes0) + bytearray(1 << 16)
        self.file_size = len(self.bytes0)
        self.h = np.frombuffer(self.buf, CACHE_HEADER, 1)[0]
        h = self.h
        types = dict(SECTION_TYPES, rows=np.dtype("<u8" if int(h["rows_in_reads"]) == 1 else "<u4"))
        self.kind = "cache_fast" if int(h["rows_in_reads"]) == 1 else "cache"
        self.a = {}
        for i, s in enumerate(C_SECTIONS):
            if s in types:
                self.a[s] = np.frombuffer(self.buf, types[s], int(h["len"][i]) // types[s].itemsize, int(h["off"][i]))
        self.n = dict(nh=int(h["nh"]), n_sides=int(h["n_sides"]), n_runs=int(h["n_runs"]), n_jump=int(h["n_jump"]), n_other=len(self.a["other"]), n_rows=int(h["n_rows"]), stride=int(h["stride"]),
                      maxlen=int(h["maxlen"]), n_pos=int(h["n_pos"]), n_segs=int(h["n_segs"]), n_chain_end=int(h["n_chain_end"]), chain_str_len=int(h["len"][C_SECTIONS.index("chain_str")]),
                      reads_size=self.reads_size, n_slots=int(h["n_slots"]), n_cm=int(h["n_cm"]))

    def write(self, path=None):
        with open(path or self.path, "wb") as f:
            f.write(bytes(self.buf[:self.file_size]))

    def write_intact(self):
        with open(self.path, "wb") as f:
            f.write(self.bytes0)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
class Entry:
    """section[element].field = value on the doors named; `do` instead of the four where the damage is not one assignment.  element and value may be functions of the door."""
    def __init__(self, name, doors, verdict, section=None, element=None, field=None, value=None, do=None, why=""):
        self.name, self.doors, self.verdict, self.section, self.element, self.field, self.value, self.do, self.why = name, tuple(doors), verdict, section, element, field, value, do, why

    def apply(self, d):
        if self.do:
            return self.do(d)
        el = self.element(d) if callable(self.element) else self.element
        v = self.value(d, el) if callable(self.value) else self.value
        if self.section == "header":
            if isinstance(self.field, tuple):
                d.h[self.field[0]][self.field[1]] = v
            else:
                d.h[self.field] = v
        elif self.field is None:
            d.a[self.section][el] = v
        else:
            d.a[self.section][self.field][el] = v


BOTH = ("pairs", "cache")
TABLE = []


def E(*a, **k):
    TABLE.append(Entry(*a, **k))


def simple_hit(d):
    return d.first_hit(lambda i, w: not w["flags"] & (RUNS1 | RUNS2))


def short_hit(d):
    """a hit of a read shorter than the longest, if the unit has one (else any hit without runs: len = maxlen is then what it holds)"""
    try:
        return d.first_hit(lambda i, w: not w["flags"] & (RUNS1 | RUNS2) and w["len"] < d.n["maxlen"])
    except LookupError:
        return simple_hit(d)


def hit_for_last_side(kind):
    """a hit with runs in mate 1 (kind RUNS1), or in mate 2 only (RUNS2), that stays what it is to pass J's list when it is given the last side record"""
    def find(d):
        last = d.a["sides"][d.n["n_sides"] - 1]

        def fits(i, w):
            f = int(w["flags"])
            if (kind == RUNS1 and not f & RUNS1) or (kind == RUNS2 and (f & RUNS1 or not f & RUNS2)):
                return False
            n_last = int(last["nruns"] >> 16 if f & LEFT2 else last["nruns"] & 0xFFFF)
            left_has_runs = bool(f & (RUNS2 if f & LEFT2 else RUNS1))
            return d.is_jump(i) == (left_has_runs and n_last >= 2)
        return d.first_hit(fits)
    return find


def side_with_one_run(mate):
    """a side record whose mate `mate` has exactly one run: moved to the pool's last run it keeps its count (pass J's list does not change) and has no order to keep"""
    def find(d):
        for i, sd in enumerate(d.a["sides"]):
            if int(sd["nruns"] & 0xFFFF if mate == 1 else sd["nruns"] >> 16) == 1:
                return i
        raise LookupError("no side record with one run in mate %d" % mate)
    return find


# -- hits
E("hit_row_n_rows", BOTH, "hit_row", "hits", 0, "row", lambda d, e: d.n["n_rows"])
E("hit_row_last", BOTH, ACCEPTED, "hits", 0, "row", lambda d, e: d.n["n_rows"] - 1)
E("hit_len_0", BOTH, "hit_len", "hits", simple_hit, "len", 0)
E("hit_len_maxlen", BOTH, ACCEPTED, "hits", short_hit, "len", lambda d, e: d.n["maxlen"], why="a mate without runs, far from the unit's end: no other rule looks at its length")
E("hit_len_maxlen_plus_1", BOTH, "hit_len", "hits", short_hit, "len", lambda d, e: d.n["maxlen"] + 1)
E("hit0_back_0", BOTH, ACCEPTED, "hits", 0, "back", 0)
E("hit0_back_1", BOTH, "hit_back", "hits", 0, "back", 1)
E("hit1_back_1", BOTH, ACCEPTED, "hits", 1, "back", 1)
E("hit1_back_2", BOTH, "hit_back", "hits", 1, "back", 2)
E("hit_side_runs1_n_sides", BOTH, "hit_side", "hits", hit_for_last_side(RUNS1), "a", lambda d, e: d.n["n_sides"])
E("hit_side_runs1_last", BOTH, ACCEPTED, "hits", hit_for_last_side(RUNS1), "a", lambda d, e: d.n["n_sides"] - 1)
E("hit_side_runs2_n_sides", BOTH, "hit_side", "hits", hit_for_last_side(RUNS2), "b", lambda d, e: d.n["n_sides"])
E("hit_side_runs2_last", BOTH, ACCEPTED, "hits", hit_for_last_side(RUNS2), "b", lambda d, e: d.n["n_sides"] - 1)
# -- sides
E("side_runs1_end_n_runs", BOTH, ACCEPTED, "sides", side_with_one_run(1), "runs1", lambda d, e: d.n["n_runs"] - 1)
E("side_runs1_end_n_runs_plus_1", BOTH, "side_runs", "sides", side_with_one_run(1), "runs1", lambda d, e: d.n["n_runs"])
E("side_runs2_end_n_runs", BOTH, ACCEPTED, "sides", side_with_one_run(2), "runs2", lambda d, e: d.n["n_runs"] - 1)
E("side_runs2_end_n_runs_plus_1", BOTH, "side_runs", "sides", side_with_one_run(2), "runs2", lambda d, e: d.n["n_runs"])


# -- jump list
def jump_drop(d):
    j, n = d.a["jump"], d.n["n_jump"]
    j[0:n - 1] = j[1:n].copy()
    j[n - 1] = 0              # (what a section one entry short reads as: the padding)


def jump_swap(d):
    j = d.a["jump"]
    j[0], j[1] = int(j[1]), int(j[0])


def jump_name_hit(one_run):
    """an entry replaced by a hit between its neighbours (the order holds) whose left mate has exactly one run (a clip: it has a side record), or none at all"""
    def do(d):
        j, n = d.a["jump"], d.n["n_jump"]
        for i in range(1, n - 1):
            for h in range(int(j[i - 1]) + 1, int(j[i + 1])):
                w = d.a["hits"][h]
                has = bool(w["flags"] & (RUNS2 if w["flags"] & LEFT2 else RUNS1))
                if not d.is_jump(h) and has == one_run and (not one_run or d.mate_runs(h, 2 if w["flags"] & LEFT2 else 1)[1] == 1):
                    j[i] = h
                    return
        raise LookupError("no such hit in a gap of pass J's list")
    return do


E("jump_entry_dropped", BOTH, "jump_order", do=jump_drop, why="the count still agrees with the hits; the zero read in the last place is not above its neighbour")
E("jump_entry_nh", BOTH, "jump_entry", "jump", 0, None, lambda d, e: d.n["nh"])
E("jump_entries_swapped", BOTH, "jump_order", do=jump_swap)
E("jump_names_single_run_hit", BOTH, "jump_hit", do=jump_name_hit(True))
E("jump_names_hit_without_runs", BOTH, "jump_hit", do=jump_name_hit(False))
E("jump_count_minus_1", BOTH, "jump_count", do=lambda d: d.set_count("n_jump", d.n["n_jump"] - 1))


# -- other bases
def other_swap(d):
    o = d.a["other"]
    o[0], o[1] = int(o[1]), int(o[0])


E("other_entry_n_bases", BOTH, "other_in_rows", "other", lambda d: d.n["n_other"] - 1, None, lambda d, e: d.n["n_rows"] * d.n["stride"])
E("other_entry_last_base", BOTH, ACCEPTED, "other", lambda d: d.n["n_other"] - 1, None, lambda d, e: d.n["n_rows"] * d.n["stride"] - 1, why="the list's last entry: the order holds")
E("other_entries_swapped", ("pairs",), "other_order", do=other_swap)
E("other_entries_swapped_cache_with_read_bases", ("cache",), ACCEPTED, do=other_swap, why="a cache that carries the reads' bases never bisects the list (rows_in_reads != 2): load_cache asks for the order only where the walk uses it")


# -- what the code reading suspected and the sanitizer run (tests/damaged_inputs_san.cpp) decided: each on a hit whose left mate is forward and on one whose left mate is reverse
def left_strand(w):
    return bool(w["flags"] & (REV2 if w["flags"] & LEFT2 else REV1))


def first_hit_on_strand(d, rev, pred):
    """The first hit pred holds for, its left mate on the given strand.  Aligners put the left mate on the forward strand: for the reverse case the hit found has both its
    strand bits turned (no rule judges them, the mates stay on opposite strands), so that the device would read its bases from the row's far end (len - 1 - q)."""
    i = d.first_hit(lambda i, w: pred(i, w) and not left_strand(w))
    if rev:
        d.a["hits"]["flags"][i] ^= REV1 | REV2
    return i


def hit_left_runs(rev, min_runs=1):
    """a hit whose left mate has runs, on the given strand, with a simple other mate"""
    def find(d):
        def fits(i, w):
            f = int(w["flags"])
            lbit, obit = (RUNS2, RUNS1) if f & LEFT2 else (RUNS1, RUNS2)
            return bool(f & lbit) and not f & obit and d.mate_runs(i, 2 if f & LEFT2 else 1)[1] >= min_runs
        return first_hit_on_strand(d, rev, fits)
    return find


def last_left_run(rev):
    def find(d):
        i = hit_left_runs(rev)(d)
        first, n = d.mate_runs(i, 2 if d.a["hits"][i]["flags"] & LEFT2 else 1)
        d.picked_hit = i
        return first + n - 1
    return find


def run_to_read_end(plus):
    return lambda d, e: int(d.a["hits"]["len"][d.picked_hit]) - int(d.a["runs"]["q"][e]) + plus


def hit_simple_other(rev):
    """a hit whose OTHER mate (not the left one) is one full-length run, its left mate on the given strand"""
    def find(d):
        return first_hit_on_strand(d, rev, lambda i, w: not w["flags"] & (RUNS1 if w["flags"] & LEFT2 else RUNS2))
    return find


def other_mate_end(plus):
    """the other mate moved so that its last base lies on position n_pos - 1 + plus"""
    def do_for(rev):
        def do(d):
            i = hit_simple_other(rev)(d)
            w = d.a["hits"][i]
            d.a["hits"]["a" if w["flags"] & LEFT2 else "b"][i] = d.n["n_pos"] - int(w["len"]) + plus
        return do
    return do_for


def other_mate_run_end(plus):
    """the same for an other mate with runs: its last run moved"""
    def do(d):
        def fits(i, w):
            return bool(w["flags"] & (RUNS1 if w["flags"] & LEFT2 else RUNS2))
        i = d.first_hit(fits)
        first, n = d.mate_runs(i, 1 if d.a["hits"][i]["flags"] & LEFT2 else 2)
        r = d.a["runs"]
        r["t"][first + n - 1] = d.n["n_pos"] - int(r["n"][first + n - 1]) + plus
    return do


def run_into_next(d):
    """a run that ends where the next begins in the read (a deletion lies between them): one longer and they overlap"""
    r = d.a["runs"]
    for sd in d.a["sides"]:
        for first, n in ((int(sd["runs1"]), int(sd["nruns"] & 0xFFFF)), (int(sd["runs2"]), int(sd["nruns"] >> 16))):
            for j in range(first, first + n - 1):
                if int(r["q"][j]) + int(r["n"][j]) == int(r["q"][j + 1]) and int(r["n"][j]):
                    r["n"][j] += 1
                    return
    raise LookupError("no deletion between two runs")


def run_onto_next(d):
    """a run that ends where the next begins on the reference (an insertion lies between them): moved up by one position and they overlap there"""
    r = d.a["runs"]
    for sd in d.a["sides"]:
        for first, n in ((int(sd["runs1"]), int(sd["nruns"] & 0xFFFF)), (int(sd["runs2"]), int(sd["nruns"] >> 16))):
            for j in range(first, first + n - 1):
                if int(r["t"][j]) + int(r["n"][j]) == int(r["t"][j + 1]) and int(r["n"][j]) and int(r["q"][j]) + int(r["n"][j]) < int(r["q"][j + 1]):
                    r["t"][j] += 1
                    return
    raise LookupError("no insertion between two runs")


def runs_swapped(d):
    r = d.a["runs"]
    for sd in d.a["sides"]:
        first, n = int(sd["runs1"]), int(sd["nruns"] & 0xFFFF)
        if n >= 2 and int(r["n"][first]) and int(r["n"][first + 1]):
            a, b = r[first].copy(), r[first + 1].copy()
            r[first], r[first + 1] = b, a
            return
    raise LookupError("no mate with two runs")


for _rev, _s in ((False, "forward"), (True, "reverse")):
    E("run_ends_at_read_end_" + _s, BOTH, ACCEPTED, "runs", last_left_run(_rev), "n", run_to_read_end(0), why="the mate's last run: nothing behind it to run into")
    E("run_ends_past_read_end_" + _s, BOTH, "run_in_read", "runs", last_left_run(_rev), "n", run_to_read_end(1))
    E("other_mate_ends_at_unit_end_" + _s, BOTH, ACCEPTED, do=other_mate_end(0)(_rev))
    E("other_mate_ends_past_unit_end_" + _s, BOTH, "mate_in_unit", do=other_mate_end(1)(_rev))
    for _bit in (32, 64, 128):
        E("hit_flag_bit_%d_%s" % (_bit, _s), BOTH, "hit_flags", "hits", hit_simple_other(_rev), "flags", lambda d, e, _bit=_bit: int(d.a["hits"]["flags"][e]) | _bit)
E("other_mate_run_ends_at_unit_end", BOTH, ACCEPTED, do=other_mate_run_end(0), why="its last run moves up the reference: the order holds")
E("other_mate_run_ends_past_unit_end", BOTH, "mate_in_unit", do=other_mate_run_end(1))
E("run_one_longer_into_the_next", BOTH, "run_order", do=run_into_next)
E("run_moved_onto_the_next", BOTH, "run_order", do=run_onto_next)
E("runs_of_a_mate_swapped", BOTH, "run_order", do=runs_swapped)


# -- cache only: conti-mer runs, counts, chain ends, rows
def seg_at_unit_end(plus):
    """a run moved to the unit's last positions (the ones appended for contig insertions carry conti-mers): one whose rank stays below the counts it then lies on"""
    def do(d):
        g, cnt, n_pos = d.a["segs"], d.a["cm_cnt"], d.n["n_pos"]
        for i in range(len(g)):
            n = int(g["len"][i])
            if n and int(cnt[n_pos - n:].min()) > int(g["rank"][i]):
                g["pos0"][i] = n_pos - n + plus
                return
        raise LookupError("no run fits the unit's last positions")
    return do


def covered_position(d):
    g = d.a["segs"][0]
    return int(g["pos0"])


def seg_min_count(d, e):
    g = d.a["segs"][e]
    return int(d.a["cm_cnt"][int(g["pos0"]):int(g["pos0"]) + int(g["len"])].min())


E("seg_end_n_pos", ("cache",), ACCEPTED, do=seg_at_unit_end(0))
E("seg_end_n_pos_plus_1", ("cache",), "seg_span", do=seg_at_unit_end(1))
E("seg_hop_end_last", ("cache",), ACCEPTED, "segs", 0, "hop_end", lambda d, e: d.n["n_pos"] - 1)
E("seg_hop_end_n_pos", ("cache",), "seg_hop_end", "segs", 0, "hop_end", lambda d, e: d.n["n_pos"])
E("seg_hop_str_at_bound", ("cache",), ACCEPTED, "segs", 0, "hop_len0", lambda d, e: d.n["chain_str_len"] + 1 - int(d.a["segs"]["hop_str0"][e]))
E("seg_hop_str_past_bound", ("cache",), "seg_hop_str", "segs", 0, "hop_len0", lambda d, e: d.n["chain_str_len"] + 2 - int(d.a["segs"]["hop_str0"][e]))
E("seg_elem0_plus_1", ("cache",), "seg_elem0", "segs", 1, "elem0", lambda d, e: int(d.a["segs"]["elem0"][e]) + 1)
E("seg_elem0_minus_1", ("cache",), "seg_elem0", "segs", 1, "elem0", lambda d, e: int(d.a["segs"]["elem0"][e]) - 1)
E("seg_len_plus_1", ("cache",), "seg_elem0", "segs", 0, "len", lambda d, e: int(d.a["segs"]["len"][e]) + 1, why="the next run no longer starts where this one ends")
E("last_seg_len_minus_1", ("cache",), "cm_total", "segs", lambda d: d.n["n_segs"] - 1, "len", lambda d, e: int(d.a["segs"]["len"][e]) - 1, why="no run behind it: the elements no longer add up to the header's conti-mers")
E("cm_cnt_plus_1", ("cache",), "cm_sum", "cm_cnt", covered_position, None, lambda d, e: int(d.a["cm_cnt"][e]) + 1)
E("cm_cnt_minus_1", ("cache",), "seg_rank", "cm_cnt", covered_position, None, lambda d, e: int(d.a["cm_cnt"][e]) - 1, why="a position's count is its highest rank + 1: one less and a run's rank is no longer below it")
E("cm_cnt_uncovered_plus_1", ("cache",), "cm_sum", "cm_cnt", lambda d: int(np.flatnonzero(d.a["cm_cnt"] == 0)[0]), None, 1)
E("seg_rank_count_minus_1", ("cache",), ACCEPTED, "segs", 0, "rank", lambda d, e: seg_min_count(d, e) - 1)
E("seg_rank_count", ("cache",), "seg_rank", "segs", 0, "rank", seg_min_count)
E("seg_rank_255", ("cache",), "seg_rank", "segs", 0, "rank", 255)
E("chain_end_last", ("cache",), ACCEPTED, "chain_end", 0, None, lambda d, e: d.n["n_pos"] - 1)
E("chain_end_n_pos", ("cache",), "chain_end", "chain_end", 0, None, lambda d, e: d.n["n_pos"])
E("row_slot_last", ("cache",), ACCEPTED, "rows", 0, None, lambda d, e: d.n["n_slots"] - 1)
E("row_slot_n_slots", ("cache",), "row_slot", "rows", 0, None, lambda d, e: d.n["n_slots"])
E("row_offset_last", ("cache_fast",), ACCEPTED, "rows", 0, None, lambda d, e: d.n["reads_size"] - d.n["maxlen"])
E("row_offset_past", ("cache_fast",), "row_offset", "rows", 0, None, lambda d, e: d.n["reads_size"] - d.n["maxlen"] + 1)
E("row_offset_wraps", ("cache_fast",), "row_offset", "rows", 0, None, (1 << 64) - 1, why="offset + maxlen wraps to a small number: the second clause")


# -- headers.  A length / count pair disagrees by one element; a count beyond its partner; a layout of another build.
def H(name, doors, verdict, field, value, **k):
    E(name, doors, verdict, "header", None, field, value, **k)


def bump(field, by=1):
    return lambda d, e: int(d.h[field[0]][field[1]] if isinstance(field, tuple) else d.h[field]) + by


def plen(s):
    return ("len", P_SECTIONS.index(s))


def clen(s):
    return ("len", C_SECTIONS.index(s))


def count_beyond_hits(name, sections):
    """n_sides / n_jump = nh + 1 with the section's length to match (the file made longer where the section is its last)"""
    def do(d):
        sec = {"n_sides": "sides", "n_jump": "jump"}[name]
        i = sections.index(sec)
        d.h[name] = int(d.h["nh"]) + 1
        d.h["len"][i] = (int(d.h["nh"]) + 1) * SECTION_TYPES[sec].itemsize
        d.file_size = max(d.file_size, int(d.h["off"][i]) + int(d.h["len"][i]))
    return do


PH, CH = ("pairs",), ("cache_header",)
H("pairs_magic", PH, "magic", ("magic", 7), ord("2"))
H("pairs_version", PH, "version", "version", 2)
H("pairs_sizes_hit", PH, "sizes", ("sizes", 0), 20)
H("pairs_sizes_side", PH, "sizes", ("sizes", 1), 16)
H("pairs_sizes_run", PH, "sizes", ("sizes", 2), 12)
H("pairs_k", PH, "k", "k", bump("k"))
H("pairs_batch", PH, "batch", "batch", bump("batch"))
H("pairs_section_past_the_file", PH, "section_bounds", ("off", 0), lambda d, e: d.file_size + 1)
H("pairs_section_longer_than_the_file", PH, "section_bounds", plen("codes"), lambda d, e: d.file_size)
H("pairs_nh_2_32", PH, "count_limits", "nh", 0xFFFFFFFF)
H("pairs_n_runs_2_32", PH, "count_limits", "n_runs", 0xFFFFFFFF)
H("pairs_n_rows_2_31", PH, "count_limits", "n_rows", 0x7FFFFFFF)
H("pairs_nh_plus_1", PH, "len_hits", "nh", bump("nh"))
H("pairs_n_sides_plus_1", PH, "len_sides", "n_sides", bump("n_sides"))
H("pairs_n_runs_plus_1", PH, "len_runs", "n_runs", bump("n_runs"))
H("pairs_n_codes_plus_1", PH, "len_codes", "n_codes", bump("n_codes"))
H("pairs_n_other_plus_1", PH, "len_other", "n_other", bump("n_other"))
H("pairs_len_otherb_plus_1", PH, "len_otherb", plen("otherb"), bump(plen("otherb")))
H("pairs_n_jump_plus_1", PH, "len_jump", "n_jump", bump("n_jump"))
H("pairs_stride_plus_1", PH, "stride_mod4", "stride", bump("stride"))
H("pairs_maxlen_stride_plus_1", PH, "maxlen_stride", "maxlen", lambda d, e: int(d.h["stride"]) + 1)
H("pairs_maxlen_stride", PH, ACCEPTED, "maxlen", lambda d, e: int(d.h["stride"]))
H("pairs_n_rows_plus_1", PH, "codes_rows", "n_rows", bump("n_rows"))
E("pairs_n_sides_beyond_hits", PH, "sides_hits", do=count_beyond_hits("n_sides", P_SECTIONS))
E("pairs_n_jump_beyond_hits", PH, "jump_hits", do=count_beyond_hits("n_jump", P_SECTIONS))

H("cache_magic", CH, "magic", ("magic", 7), ord("6"))
H("cache_version", CH, "version", "version", 3)
H("cache_batch", CH, "batch", "batch", bump("batch"))
H("cache_k", CH, "k", "k", bump("k"))
for _i, _v in enumerate((20, 12, 44, 520, 16)):
    H("cache_sizes_%d" % _i, CH, "sizes", ("sizes", _i), _v)
H("cache_section_past_the_file", CH, "section_bounds", ("off", 0), lambda d, e: d.file_size + 1)
H("cache_section_longer_than_the_file", CH, "section_bounds", clen("codes"), lambda d, e: d.file_size)
H("cache_rows_in_reads_3", CH, "rows_in_reads", "rows_in_reads", 3)
H("cache_n_pos_0", CH, "n_pos", "n_pos", 0)
H("cache_nh_2_32", CH, "count_limits", "nh", 0xFFFFFFFF)
H("cache_n_runs_2_32", CH, "count_limits", "n_runs", 0xFFFFFFFF)
H("cache_n_rows_2_31", CH, "count_limits", "n_rows", 0x7FFFFFFF)
H("cache_n_pos_2_32", CH, "n_pos", "n_pos", 0xFFFFFF00)
H("cache_n_ref_beyond_n_pos", CH, "n_ref", "n_ref", lambda d, e: int(d.h["n_pos"]) + 1)
H("cache_n_ref_n_pos", CH, ACCEPTED, "n_ref", lambda d, e: int(d.h["n_pos"]))
H("cache_len_ref_minus_1", CH, "len_ref", clen("ref"), bump(clen("ref"), -1))
H("cache_len_cm_cnt_minus_1", CH, "len_cm_cnt", clen("cm_cnt"), bump(clen("cm_cnt"), -1))
H("cache_nh_plus_1", CH, "len_hits", "nh", bump("nh"))
H("cache_n_runs_plus_1", CH, "len_runs", "n_runs", bump("n_runs"))
H("cache_n_sides_plus_1", CH, "len_sides", "n_sides", bump("n_sides"))
E("cache_n_sides_beyond_hits", CH, "sides_hits", do=count_beyond_hits("n_sides", C_SECTIONS))
H("cache_n_jump_plus_1", CH, "len_jump", "n_jump", bump("n_jump"))
E("cache_n_jump_beyond_hits", CH, "jump_hits", do=count_beyond_hits("n_jump", C_SECTIONS))
H("cache_n_codes_plus_1", CH, "len_codes", "n_codes", bump("n_codes"))
H("cache_n_segs_plus_1", CH, "len_segs", "n_segs", bump("n_segs"))
H("cache_n_seg0_beyond_segs", CH, "seg0_segs", "n_seg0", lambda d, e: int(d.h["n_segs"]) + 1)
H("cache_len_rows_plus_1_row", CH, "len_rows", clen("rows"), bump(clen("rows"), 4))
H("cache_stride_plus_1", CH, "stride_mod4", "stride", bump("stride"))


def cache_otherb_one_byte(d):
    i = C_SECTIONS.index("otherb")
    d.h["len"][i] = 1
    d.file_size = int(d.h["off"][i]) + 4096


def cache_rows_plus_1(d):
    d.h["n_rows"] = int(d.h["n_rows"]) + 1
    d.h["len"][C_SECTIONS.index("rows")] += 4


def cache_slot_stride_below_maxlen(d):
    d.h["slot_stride"] = int(d.h["maxlen"]) - 1
    d.h["len"][C_SECTIONS.index("bases")] = int(d.h["n_slots"]) * (int(d.h["maxlen"]) - 1)


E("cache_len_otherb_with_read_bases", CH, "len_otherb", do=cache_otherb_one_byte)
H("cache_n_slots_plus_1", CH, "len_bases", "n_slots", bump("n_slots"))
H("cache_n_chain_end_plus_1", CH, "len_chain_end", "n_chain_end", bump("n_chain_end"))
E("cache_n_rows_plus_1", CH, "codes_rows", do=cache_rows_plus_1)
H("cache_len_other_plus_1_byte", CH, "len_other", clen("other"), bump(clen("other")))
H("cache_maxlen_stride_plus_1", CH, "maxlen_stride", "maxlen", lambda d, e: int(d.h["stride"]) + 1)
E("cache_slot_stride_below_maxlen", CH, "maxlen_slot_stride", do=cache_slot_stride_below_maxlen)

BY_NAME = {e.name: e for e in TABLE}
assert len(BY_NAME) == len(TABLE)
