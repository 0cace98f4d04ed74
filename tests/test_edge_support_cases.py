"""agx_support_lane (csrc/agx_core.h), the lane function of agx_k_edge_support, on the CPU: tests/edge_support_shim.cpp runs it serially over every (tile list entry,
lane) and tests/edge_support_model.py — the reference's loop over read indices, nothing of the engine — says how many events must name each edge.  The node and edge
tables are the oracle's, laid out as the device's with canonical ids as slots: a node's first four successors inline, the rest on an overflow list that names every
second pair twice, in a shuffled order.  Units: every case of tests/edge_units.py and tests/lean_units.py (without the two 65 535-entry pile-ups) and the generated
seeds 201 and 203.  Both forms of the lane function run: with the single -> single shortcut (the kernel's) and with every position resolved through its candidate keys.
tests/test_gpu_edge_support.py runs the kernel itself on the same units and imports them from here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edge_support_model as ESM
import edge_units as EU
import harness as H
import lean_units as LU
from hostsim import sim
from test_gpu_parity import CONFIGS

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "edge_support_shim.cpp")
MAXE, EOVF = 4, 4      # AGX_MAXE, AGX_NF_EOVF (agx_core.h)
SEEDS = (201, 203)


class SupportUnit:
    def __init__(self, name, k, iv, coverage, write, windows=False, overflow=False):
        """write(dir) -> tmp/ directory of the unit's files"""
        self.name, self.k, self.iv, self.coverage, self.write, self.windows, self.overflow = name, k, iv, coverage, write, windows, overflow


def _synth_unit(seed):
    cfg = next(c for c in CONFIGS if c["seed"] == seed)

    def write(d):
        return os.path.join(H.synth(os.path.join(d, "run"), sam_seq=0, **cfg), "tmp")
    return SupportUnit("seed%d" % seed, cfg.get("k", 5), cfg.get("insert_variation", 50), cfg["coverage"], write)


EDGE_UNITS = [SupportUnit("edge_" + c.name, LU.K, c.iv, c.coverage, lambda d, c=c: LU.write_unit(c.unit, d), windows=c.windows, overflow=c.overflow) for c in EU.cases()]
LEAN_UNITS = [SupportUnit("lean_" + c.name, LU.K, LU.IV, 1, lambda d, c=c: LU.write_unit(c.unit, d)) for c in LU.cases(slow=False)]
SEED_UNITS = [_synth_unit(s) for s in SEEDS]
UNITS = {u.name: u for u in EDGE_UNITS + LEAN_UNITS + SEED_UNITS}


@pytest.fixture(scope="module")
def modelled(built, tmp_path_factory):
    """name -> (unit, tmp, oracle graph, front in file order, the model's support): made once per module"""
    made = {}

    def get(name):
        if name not in made:
            u = UNITS[name]
            tmp = u.write(str(tmp_path_factory.mktemp(name)))
            if name.startswith("seed"):
                meta = H.read_meta(os.path.dirname(tmp))
                assert (meta["k"], meta["insert_variation"], meta["coverage"]) == (u.k, u.iv, u.coverage)
            g = H.run_oracle(tmp, 0, u.k, u.iv, u.coverage, graph=True)["graph"]
            front = sim.run(tmp, 0, u.k, u.iv, u.coverage, front=True)["front"]
            made[name] = (u, tmp, g, front, ESM.support(front, g, u.k, u.iv))
        return made[name]
    return get


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("edge_support_shim") / "libedge_support_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SHIM])
    L = ctypes.CDLL(so)
    L.agx_edge_support_shim.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def device_tables(g, model):
    """The oracle's tables as the device's: n_next (four inline slots per node, NONE behind the last), the overflow list (pairs beyond the fourth, every second one twice,
    shuffled), the EOVF flags; and for every edge of the model's order where its counter is: (inline word index, -1) or (-1, the pair's entries on the list)."""
    nn = int(g["n_nodes"])
    es, ed = model["edge_start"].astype(np.int64), model["edge_dst"].astype(np.int64)
    n_next = np.full(nn * MAXE, ESM.NONE, np.uint32)
    flags = np.zeros(max(nn, 1), np.uint8)
    spill = []
    for c in np.nonzero(np.diff(es) > 0)[0]:
        lo, hi = int(es[c]), int(es[c + 1])
        n_next[c * MAXE:c * MAXE + min(MAXE, hi - lo)] = ed[lo:min(hi, lo + MAXE)]
        if hi - lo > MAXE:
            flags[c] |= EOVF
            spill += [(int(c), int(d)) for d in ed[lo + MAXE:hi]]
    lst = spill + spill[::2]
    np.random.RandomState(5).shuffle(lst)
    ovf = np.array(lst, np.uint32).reshape(-1, 2)
    return n_next, flags, ovf


def edge_counts(model, e_cnt, ovf, ovf_cnt):
    """Counters in the device's layout -> one number per edge of the model's order (overflow duplicates summed)."""
    es, ed = model["edge_start"].astype(np.int64), model["edge_dst"].astype(np.int64)
    on_list = {}
    for (s, d), n in zip(ovf.tolist(), ovf_cnt.tolist()):
        on_list[(s, d)] = on_list.get((s, d), 0) + n
    out = np.zeros(len(ed), np.int64)
    owner = np.repeat(np.arange(len(es) - 1), np.diff(es))
    rank = np.arange(len(ed)) - es[owner]
    inline = rank < MAXE
    out[inline] = e_cnt[owner[inline] * MAXE + rank[inline]]
    for e in np.nonzero(~inline)[0]:
        out[e] = on_list[(int(owner[e]), int(ed[e]))]
    return out


def run_shim(shim, u, g, front, model, single_ok):
    n_pos, nn = int(g["n_pos"]), int(g["n_nodes"])
    n_next, flags, ovf = device_tables(g, model)
    ns = g["node_start"].astype(np.int64)
    node_start = np.ascontiguousarray(ns[:n_pos], np.uint32)
    node_cnt = np.ascontiguousarray(np.diff(ns), np.uint16)
    nk = np.ascontiguousarray(g["node_key"][:, [0, 1, 2, 3, 5]].T, np.uint32)
    keep = [np.ascontiguousarray(front[k]) for k in ("cm_start", "cm", "dhit", "runs", "tile_off")]
    tile_hit = np.ascontiguousarray(front["tile_recs"]["hit"], np.uint32)
    e_cnt, ovf_cnt, out = np.zeros(max(nn, 1) * MAXE, np.uint32), np.zeros(max(len(ovf), 1), np.uint32), np.zeros(3, np.uint64)
    ovf_c = np.ascontiguousarray(ovf if len(ovf) else np.zeros((1, 2), np.uint32))

    def p(a):
        return a.ctypes.data
    rc = shim.agx_edge_support_shim(p(keep[0]), p(keep[1]), p(keep[2]), len(keep[2]), p(keep[3]), p(keep[4]), p(tile_hit), n_pos, u.k, u.iv,
                                    p(node_start), p(node_cnt), p(nk), nn, p(n_next), p(flags), p(ovf_c), len(ovf), 1 if single_ok else 0, p(e_cnt), p(ovf_cnt), p(out))
    assert rc == 0
    return {"edge_cnt": edge_counts(model, e_cnt, ovf, ovf_cnt[:len(ovf)]), "n_events": int(out[0]), "n_contributions": int(out[1]), "unmatched": int(out[2]),
            "ovf": ovf, "ovf_cnt": ovf_cnt[:len(ovf)]}


@pytest.mark.parametrize("name", list(UNITS))
def test_lane_function_matches_model(shim, modelled, name):
    u, tmp, g, front, model = modelled(name)
    assert model["off_graph"] == 0, "the model names a pair that is no edge of the oracle's graph"
    assert len(model["edge_cnt"]) == int(g["n_edges"]) and (model["edge_cnt"] >= 1).all(), "an edge of the oracle's graph without an event"
    fast = run_shim(shim, u, g, front, model, True)
    slow = run_shim(shim, u, g, front, model, False)
    for got in (fast, slow):
        assert got["unmatched"] == 0
        assert got["n_events"] == model["n_events"] and got["n_contributions"] == model["n_contributions"]
        assert np.array_equal(got["edge_cnt"], model["edge_cnt"].astype(np.int64))
        assert (got["edge_cnt"] >= 1).all()
    assert np.array_equal(fast["ovf_cnt"], slow["ovf_cnt"])
    if u.overflow:      # the first entry of a pair takes its counts, a duplicate none
        assert len(fast["ovf"]) > len(np.unique(fast["ovf"], axis=0)) and (fast["ovf_cnt"] == 0).any() and fast["ovf_cnt"].sum() > 0


def test_units_reach_both_forms(modelled):
    """Some unit has positions with one variant on both sides of a step (the shortcut) and some has several on either side, overflow edges and chain events."""
    u, tmp, g, front, model = modelled("edge_register")
    per_pos = np.diff(g["node_start"].astype(np.int64))
    assert (per_pos == 1).any() and (per_pos >= 4).any()
    E = ESM.events(modelled("lean_general")[3], LU.K)
    assert (E[:, 2] == ESM.NONE).any() and (E[:, 3] == ESM.NONE).any(), "no event without a mate position (the chains of a read insertion next to a gap)"
    assert any(UNITS[n].overflow for n in UNITS)
