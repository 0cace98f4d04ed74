"""agx_reads_lane (csrc/agx_core.h), the lane function of agx_k_edge_reads, on the CPU: tests/edge_reads_shim.cpp runs it serially over every (tile list entry, lane) with a
recording put, inside a serial replay of the count / scan / emit offsets and of the chunk loop, and tests/edge_reads_model.py says which hits must stand behind which
edge.  Tables, units and layout are those of tests/test_edge_support_cases.py (the oracle's node and edge tables as the device's, an overflow list with duplicates, every
case of tests/edge_units.py and tests/lean_units.py and the seeds 201 and 203); the counters the filter reads are filled by tests/edge_support_shim.cpp from the same
tables.  The derived records are handed over in a shuffled order with its perm[], so a record that carries a place instead of a file number is seen.  Both forms of the
lane function run: with the single -> single shortcut and without."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edge_reads_model as ERM
from test_edge_support_cases import HERE, MAXE, SHIM, UNITS, device_tables, modelled  # noqa: F401  (modelled: the module fixture)

READS_SHIM = os.path.join(HERE, "edge_reads_shim.cpp")
ALL = ERM.ALL
BIG = 1 << 40


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("edge_reads_shim") / "libedge_reads_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, READS_SHIM, SHIM])
    L = ctypes.CDLL(so)
    tables = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    nodes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]
    L.agx_edge_support_shim.argtypes = tables + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int] + nodes + [ctypes.c_void_p] * 3
    L.agx_edge_reads_shim.argtypes = tables + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int] + nodes + \
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


class Laid:
    """A unit's arrays as the shims take them, the counters counted once"""

    def __init__(self, shim, u, g, front, model):
        self.shim, self.u, self.g = shim, u, g
        self.n_pos, self.nn = int(g["n_pos"]), int(g["n_nodes"])
        self.n_next, self.flags, ovf = device_tables(g, model)
        self.n_ovf = len(ovf)
        self.ovf = np.ascontiguousarray(ovf if len(ovf) else np.zeros((1, 2), np.uint32))
        ns = g["node_start"].astype(np.int64)
        self.node_start, self.node_cnt = np.ascontiguousarray(ns[:self.n_pos], np.uint32), np.ascontiguousarray(np.diff(ns), np.uint16)
        self.nk = np.ascontiguousarray(g["node_key"][:, [0, 1, 2, 3, 5]].T, np.uint32)
        self.cm_start, self.cm, self.runs, self.tile_off = (np.ascontiguousarray(front[k]) for k in ("cm_start", "cm", "runs", "tile_off"))
        # the device's order of the derived records: any order, with perm[place] = file number
        nh = len(front["dhit"])
        self.perm = np.random.RandomState(7).permutation(nh).astype(np.uint32)
        place_of = np.zeros(nh, np.uint32)
        place_of[self.perm] = np.arange(nh, dtype=np.uint32)
        self.dhit = np.ascontiguousarray(front["dhit"][self.perm])
        self.tile_hit = np.ascontiguousarray(place_of[front["tile_recs"]["hit"].astype(np.int64)], np.uint32)
        self.e_cnt, self.ovf_cnt = np.zeros(max(self.nn, 1) * MAXE, np.uint32), np.zeros(max(self.n_ovf, 1), np.uint32)
        out = np.zeros(3, np.uint64)
        assert shim.agx_edge_support_shim(*self._tables(), self.n_pos, u.k, u.iv, *self._nodes(True), self.e_cnt.ctypes.data, self.ovf_cnt.ctypes.data, out.ctypes.data) == 0
        assert int(out[2]) == 0 and int(out[1]) == model["n_contributions"]
        self.n_contributions = int(out[1])

    def _tables(self):
        return [a.ctypes.data for a in (self.cm_start, self.cm, self.dhit)] + [len(self.dhit), self.runs.ctypes.data, self.tile_off.ctypes.data, self.tile_hit.ctypes.data]

    def _nodes(self, single_ok):
        return [self.node_start.ctypes.data, self.node_cnt.ctypes.data, self.nk.ctypes.data, self.nn, self.n_next.ctypes.data, self.flags.ctypes.data, self.ovf.ctypes.data,
                self.n_ovf, 1 if single_ok else 0]

    def run(self, lo, hi, max_support, single_ok=True, chunk=0, room=BIG, perm=None):
        cap = self.n_contributions + 8
        recs, out = np.zeros(4 * cap, np.uint32), np.zeros(5, np.uint64)
        perm = self.perm if perm is None else perm
        rc = self.shim.agx_edge_reads_shim(*self._tables(), perm.ctypes.data, self.n_pos, self.u.k, self.u.iv, *self._nodes(single_ok), self.e_cnt.ctypes.data,
                                           self.ovf_cnt.ctypes.data, lo, hi, max_support, chunk, room, recs.ctypes.data, cap, out.ctypes.data)
        return rc, recs[:4 * int(out[0])].reshape(-1, 4), {"records": int(out[0]), "chunks": int(out[1]), "events": int(out[2]), "bad": int(out[3]), "disagree": int(out[4])}


def grouped(recs):
    """The host's part (agx_unit_edge_reads): the records grouped per edge, stable; support is the group's size here (the engine attaches the counter and compares)."""
    sv, dv = recs[:, 2] & 0xFFFF, recs[:, 2] >> 16
    order = np.lexsort((dv, recs[:, 1], sv, recs[:, 0]))      # (stable: a position's records keep the order they were emitted in)
    r, sv, dv = recs[order], sv[order], dv[order]
    key = np.stack([r[:, 0], sv, r[:, 1], dv], axis=1)
    first = np.ones(len(r), bool)
    first[1:] = (key[1:] != key[:-1]).any(axis=1)
    at = np.nonzero(first)[0]
    out = {k: key[at, j].astype(np.uint32) for j, k in enumerate(ERM.EDGE_KEYS[:4])}
    out["hit_off"] = np.concatenate([at, [len(r)]]).astype(np.uint64)
    out["support"] = np.diff(out["hit_off"].astype(np.int64)).astype(np.uint32)
    out["hit"] = r[:, 3].astype(np.uint32)
    return out


@pytest.fixture(scope="module")
def laid(shim, modelled):
    made = {}

    def get(name):
        if name not in made:
            u, tmp, g, front, model = modelled(name)
            made[name] = (Laid(shim, u, g, front, model), ERM.reads(front, g, u.k, u.iv))
        return made[name]
    return get


def windows(n_pos):
    """(lo, hi) of the windows every unit is asked for: whole, empty, one position, lo and hi in mid-tile, lane 63 -> lane 0, the last partial tile"""
    t = max(n_pos // 128, 1) * 64
    return [(0, n_pos), (t, t), (t + 5, t + 6), (t + 1, t + 63), (t + 63, t + 65), (n_pos - n_pos % 64 - (0 if n_pos % 64 else 64), n_pos)]


@pytest.mark.parametrize("name", list(UNITS))
def test_lane_function_matches_model(laid, modelled, name):
    u, tmp, g, front, model = modelled(name)
    L, rd = laid(name)
    for single_ok in (True, False):
        rc, recs, o = L.run(0, L.n_pos, ALL, single_ok)
        assert rc == 0 and (o["bad"], o["disagree"]) == (0, 0)
        assert o["events"] == model["n_events"] and o["records"] == model["n_contributions"] and o["chunks"] == 1
        got = grouped(recs)
        assert ERM.same(got, ERM.table(rd, g)) is None, ERM.same(got, ERM.table(rd, g))
        hits = got["hit"].astype(np.int64)
        inner = np.ones(len(hits), bool)
        inner[got["hit_off"][:-1].astype(np.int64)] = False
        assert (np.diff(hits)[inner[1:]] > 0).all(), "an edge's hits do not ascend as emitted"
        for lo, hi in windows(L.n_pos):
            for top in (0, 1, 2):
                rc, recs, o = L.run(lo, hi, top, single_ok)
                assert rc == 0 and (o["bad"], o["disagree"]) == (0, 0)
                want = ERM.table(rd, g, lo, hi, top)
                assert ERM.same(grouped(recs), want) is None, (lo, hi, top, ERM.same(grouped(recs), want))


@pytest.mark.parametrize("name", list(UNITS))
def test_chunks_give_the_same_records(laid, name):
    L, rd = laid(name)
    rc, whole, o = L.run(0, L.n_pos, ALL)
    n_tiles = (L.n_pos + 63) // 64
    for chunk in (1, 2, 7):
        rc, recs, c = L.run(0, L.n_pos, ALL, chunk=chunk)
        assert rc == 0 and (c["bad"], c["disagree"]) == (0, 0) and c["chunks"] == (n_tiles + chunk - 1) // chunk and c["events"] == o["events"]
        assert np.array_equal(recs, whole)      # chunks are runs of tiles in order: the very same sequence of records
    # a room that the whole unit's records do not fit: the chunk is halved until they do
    per_tile = np.bincount(whole[:, 0] // 64, minlength=n_tiles) if len(whole) else np.zeros(n_tiles, np.int64)
    room = int(per_tile.max())
    rc, recs, c = L.run(0, L.n_pos, ALL, room=max(room, 1))
    assert rc == 0 and np.array_equal(recs, whole) and (c["bad"], c["disagree"]) == (0, 0) and c["events"] == o["events"]
    if len(whole) > room:
        assert c["chunks"] > 1
    if room > 1:      # one record less than the fullest tile needs: refused, not truncated
        assert L.run(0, L.n_pos, ALL, room=room - 1)[0] == -3


def test_filter_reads_the_first_overflow_entry(laid, modelled):
    """overflow_dup lists a pair twice: the first entry holds the pair's whole support, the duplicate 0, and the filter must ask the first."""
    L, rd = laid("edge_overflow_dup")
    u, tmp, g, front, model = modelled("edge_overflow_dup")
    ovf = L.ovf[:L.n_ovf]
    assert len(ovf) > len(np.unique(ovf, axis=0)) and (L.ovf_cnt[:L.n_ovf] == 0).any()
    on_list = {(int(s), int(d)) for s, d in ovf.tolist()}
    for top in (1, 2, ALL):
        rc, recs, o = L.run(0, L.n_pos, top)
        got, want = grouped(recs), ERM.table(rd, g, 0, L.n_pos, top)
        assert rc == 0 and o["bad"] == 0 and ERM.same(got, want) is None
    listed = [e for e in rd if e in on_list]
    assert listed and any(len(rd[e]) == 1 for e in listed)


def test_a_place_is_not_a_file_number(laid, modelled):
    """The mutation "perm dropped": with the identity in place of perm[] the records name places, and the comparison with the model sees it."""
    L, rd = laid("seed201")
    u, tmp, g, front, model = modelled("seed201")
    rc, recs, o = L.run(0, L.n_pos, ALL, perm=np.arange(len(L.perm), dtype=np.uint32))
    assert rc == 0 and ERM.same(grouped(recs), ERM.table(rd, g)) == "hit"
