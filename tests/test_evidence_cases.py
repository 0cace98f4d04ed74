"""agx_evidence_lane / agx_evidence_step (csrc/agx_core.h), the lane functions of agx_k_ev_gather, on the CPU: tests/evidence_shim.cpp runs them over every flat graph base
and replays the flag / scan / runs arithmetic and the host's merge of chunk-cut intervals; tests/evidence_model.py — numpy over the oracle's graph, the walk model's id
numbering and the edge-support model, nothing of the engine — says what must come out.  The tables are the oracle's laid out as the device's with canonical ids as slots
(tests/test_edge_support_cases.py: device_tables — four successors inline, the rest on an overflow list that names every second pair twice), the counters the support
model's, an overflow pair's count split over its entries.  Units: every case of tests/walk_units.py and the generated seeds 201 and 203, each with the stretches of a real
finish through the serial executor (tests/evidence_paths_sim.cpp: the executor with its walk keeping the stretches) and with hand-made stretch tables (hand_made below).  tests/test_gpu_evidence.py runs the kernels on the same units and imports them
from here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import edge_support_model as ESM
import evidence_model as EM
import harness as H
import lean_units as LU
import path_model as PM
import walk_model as WM
import walk_units as WU
from hostsim import sim
from test_edge_support_cases import MAXE, EOVF, device_tables
from test_gpu_parity import CONFIGS

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "evidence_shim.cpp")
NONE = EM.NONE
SEEDS = (201, 203)


PATHS_SRC = os.path.join(HERE, "evidence_paths_sim.cpp")
PATHS_LIB = os.path.join(HERE, "hostsim", "libevidence_paths_sim.so")      # beside the executor's own library, built like it (hostsim.sim.build)
_paths_lib = None


def executor_paths(tmp, unit, k, iv, coverage):
    """One unit through the serial executor with its walk keeping the stretches (tests/evidence_paths_sim.cpp): (the dict of Unit.walk_paths(), the pre-extended text)."""
    global _paths_lib
    if _paths_lib is None:
        import aligngraph_amd as A
        deps = [PATHS_SRC] + sim.DEPS
        if not os.path.exists(PATHS_LIB) or any(os.path.getmtime(PATHS_LIB) < os.path.getmtime(d) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-pthread", "-o", PATHS_LIB, PATHS_SRC] + sim.SRC[1:])
        _paths_lib = ctypes.CDLL(PATHS_LIB)
        _paths_lib.agx_evidence_paths_sim.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 4 + [ctypes.c_long, ctypes.POINTER(A.WalkPaths), ctypes.POINTER(ctypes.c_void_p),
                                                      ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p, ctypes.c_size_t]
        _paths_lib.agx_evidence_paths_sim_free.argtypes = [ctypes.POINTER(A.WalkPaths), ctypes.c_void_p]
        _paths_lib.agx_evidence_paths_sim_free.restype = None
    import aligngraph_amd as A
    q, pre, n, err = A.WalkPaths(), ctypes.c_void_p(), ctypes.c_size_t(0), ctypes.create_string_buffer(512)
    rc = _paths_lib.agx_evidence_paths_sim(tmp.encode(), unit, k, iv, coverage, 1000000, ctypes.byref(q), ctypes.byref(pre), ctypes.byref(n), err, 512)
    assert rc == 0, (rc, err.value)
    try:
        def arr(p, cnt, dt):
            return np.ctypeslib.as_array(p, shape=(cnt,)).astype(dt, copy=True) if cnt else np.zeros(0, dt)
        w = {"rec_len": arr(q.rec_len, q.n_recs, "uint64"), "st_off": arr(q.st_off, q.n_recs + 1, "uint64"), "id_first": arr(q.id_first, q.n_stretches, "uint32"),
             "id_last": arr(q.id_last, q.n_stretches, "uint32"), "base_off": arr(q.base_off, q.n_stretches, "uint64"), "joined": arr(q.joined, q.n_stretches, "uint8")}
        return w, ctypes.string_at(pre, n.value)
    finally:
        _paths_lib.agx_evidence_paths_sim_free(ctypes.byref(q), pre)


class EvidenceUnit:
    def __init__(self, name, k, iv, coverage, write, overflow=False):
        self.name, self.k, self.iv, self.coverage, self.write, self.overflow = name, k, iv, coverage, write, overflow


def _synth_unit(seed):
    cfg = next(c for c in CONFIGS if c["seed"] == seed)
    return EvidenceUnit("seed%d" % seed, cfg.get("k", 5), cfg.get("insert_variation", 50), cfg["coverage"],
                        lambda d: os.path.join(H.synth(os.path.join(d, "run"), sam_seq=0, **cfg), "tmp"))


WALK_UNITS = [EvidenceUnit("walk_" + c.name, LU.K, c.iv, c.coverage, lambda d, c=c: WU.write_unit(c.unit, d), overflow=c.group == "overflow") for c in WU.cases()]
SEED_UNITS = [_synth_unit(s) for s in SEEDS]
UNITS = {u.name: u for u in WALK_UNITS + SEED_UNITS}


def thresholds(g, coverage):
    """(min_depth, min_support) pairs every unit is asked at: nothing, the build's coverage with the default support, a depth above every node's, support alone"""
    above = int(np.asarray(g["node_cnt"]).reshape(-1, 6)[:, 0].max()) + 1 if int(g["n_nodes"]) else 1
    return [(0, 0), (coverage, 2), (above, 0), (0, 5)]


def hand_made(g, wm, node):
    """Hand-made stretch tables over a unit, the smallest shapes that can go wrong: a stretch across the 64-base wave border; one-base stretches; several records inside
    one wave with equal minima; a minimum that two offsets of one record share; a joined boundary and a joined = 0 boundary directly behind a stretch; side ids; ids
    without a node; a joined pair of ids with no edge between them; every step out of a node with more than four successors (some of them overflow edges, whichever the
    device put inline); a record without a stretch."""
    n_pos, n_ids = int(wm["n_pos"]), int(wm["n_ids"])
    has = node >= 0
    main = has[:n_pos].astype(np.int8)
    # the longest run of consecutive main ids with a node, 150 at most
    edge = np.diff(np.concatenate(([0], main, [0])))
    starts, ends = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
    best = int(np.argmax(ends - starts))
    a, L = int(starts[best]), int(min(ends[best] - starts[best], 150))
    assert L >= 6, "no run of six main ids with nodes"
    recs = [(min(L, 30) + 4, [(a, a + min(L, 30) - 1, 0, 0)]),
            (L + 4, [(a, a + L - 1, 0, 0)]),
            (5, [(a, a, 0, 0)]), (5, [(a, a, 0, 0)]), (7, [(a, a, 2, 0)]),
            (20, [(a, a + 2, 0, 0), (a, a + 2, 10, 0)]),
            (9, [(a, a + 1, 0, 0), (a + 2, a + 3, 2, 1), (a + 4, a + 4, 4, 0)])]
    if n_ids > n_pos:
        recs.append((80, [(n_pos, min(n_ids, n_pos + 70) - 1, 0, 0)]))
    absent = np.nonzero(~has[:n_pos])[0]
    if len(absent):
        x = int(absent[0])
        recs.append((12, [(x, x, 0, 0)] + ([(x - 1, x + 1, 5, 0)] if 0 < x < n_pos - 1 else [])))
    present = np.nonzero(has)[0]
    recs.append((6, [(int(present[-1]), int(present[-1]), 0, 0), (int(present[0]), int(present[0]), 1, 1)]))      # backwards: no edge leads there
    id_of = np.full(int(g["n_nodes"]) + 1, -1, np.int64)
    id_of[node[has]] = present
    es = np.asarray(g["edge_start"]).astype(np.int64)
    fans = 0
    for v in np.nonzero(np.diff(es) > MAXE)[0]:
        if id_of[v] < 0 or fans == 2:
            continue
        for t in np.unique(np.asarray(g["edge_dst"])[es[v]:es[v + 1]]):
            if id_of[t] >= 0:
                recs.append((6, [(int(id_of[v]), int(id_of[v]), 0, 0), (int(id_of[t]), int(id_of[t]), 1, 1)]))
        fans += 1
    recs.append((5, []))
    return PM.stretches(recs)


@pytest.fixture(scope="module")
def modelled(built, tmp_path_factory):
    """name -> dict(u, tmp, g, wm, node, sup, w: the executor's stretches, hand: the hand-made ones): made once per module"""
    made = {}

    def get(name):
        if name not in made:
            u = UNITS[name]
            tmp = u.write(str(tmp_path_factory.mktemp(name)))
            o = H.run_oracle(tmp, 0, u.k, u.iv, u.coverage, graph=True)
            g = o["graph"]
            s = sim.run(tmp, 0, u.k, u.iv, u.coverage, front=True)
            w, pre = executor_paths(tmp, 0, u.k, u.iv, u.coverage)
            assert s["pre"] == o["pre"] and pre == o["pre"]
            wm = WM.build(g, u.coverage)
            node = PM.id_nodes(g, u.coverage, wm)
            made[name] = {"u": u, "tmp": tmp, "g": g, "wm": wm, "node": node, "sup": ESM.support(s["front"], g, u.k, u.iv), "w": w, "pre": o["pre"]}
            made[name]["hand"] = hand_made(g, wm, node)
        return made[name]
    return get


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("evidence_shim") / "libevidence_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SHIM])
    L = ctypes.CDLL(so)
    L.agx_evidence_shim.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + \
        [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_void_p] * 9
    return L


def flat_tables(w):
    """The stretch table as the device reads it: first id, first base offset, record, exclusive prefix of the lengths (closing total), joined (closing zero)."""
    st = np.asarray(w["st_off"]).astype(np.int64)
    n_st = len(w["id_first"])
    rec = np.repeat(np.arange(len(w["rec_len"]), dtype=np.uint32), np.diff(st)) if n_st else np.zeros(0, np.uint32)
    length = np.asarray(w["id_last"]).astype(np.int64) - np.asarray(w["id_first"]).astype(np.int64) + 1
    pre = np.concatenate(([0], np.cumsum(length))).astype(np.uint32)
    join = np.concatenate((np.asarray(w["joined"], np.uint8), [0])).astype(np.uint8)
    return np.asarray(w["id_first"], np.uint32), np.asarray(w["base_off"]).astype(np.uint32), rec, pre, join


def counters(sup, n_next, ovf):
    """The support model's counts in the device's layout: e_cnt parallel to n_next; an overflow pair's count on its first entry, but one of it on a second entry."""
    es, ed, ec = sup["edge_start"].astype(np.int64), sup["edge_dst"].astype(np.int64), sup["edge_cnt"].astype(np.int64)
    e_cnt = np.zeros(len(n_next), np.uint32)
    owner = np.repeat(np.arange(len(es) - 1), np.diff(es))
    rank = np.arange(len(ed)) - es[owner]
    inline = rank < MAXE
    e_cnt[owner[inline] * MAXE + rank[inline]] = ec[inline]
    count = {(int(s), int(d)): int(c) for s, d, c in zip(owner[~inline], ed[~inline], ec[~inline])}
    ovf_cnt = np.zeros(max(len(ovf), 1), np.uint32)
    seen = {}
    for i, (s, d) in enumerate(ovf.tolist()):
        seen.setdefault((s, d), []).append(i)
    for p, at in seen.items():
        ovf_cnt[at[0]] = count[p]
        if len(at) > 1 and count[p] > 1:
            ovf_cnt[at[0]] -= 1
            ovf_cnt[at[1]] = 1
    return e_cnt, ovf_cnt


def run_shim(shim, m, w, min_depth, min_support, chunk, counted=True):
    g, sup, node = m["g"], m["sup"], m["node"]
    nn = int(g["n_nodes"])
    n_next, flags, ovf = device_tables(g, sup)
    e_cnt, ovf_cnt = counters(sup, n_next, ovf)
    ovf_c = np.ascontiguousarray(ovf if len(ovf) else np.zeros((1, 2), np.uint32))
    a_nid = np.where(node >= 0, node, NONE).astype(np.uint32)
    counts = np.ascontiguousarray(np.asarray(g["node_cnt"]).reshape(-1, 6), np.int32)
    first, base, rec, pre, join = (np.ascontiguousarray(x) for x in flat_tables(w))
    n_st, n_flat, nr = len(first), int(pre[-1]), len(w["rec_len"])
    R = [np.zeros(max(nr, 1), np.uint64) for _ in range(4)]
    depth, votes, step = (np.zeros(max(n_flat, 1), np.uint32) for _ in range(3))
    iv, out = np.zeros(5 * max(n_flat, 1), np.uint32), np.zeros(2, np.uint64)

    def p(a):
        return a.ctypes.data
    rc = shim.agx_evidence_shim(p(first), p(base), p(rec), p(pre), p(join), n_st, n_flat, p(a_nid), len(a_nid), nn, p(counts), p(n_next), p(flags), p(ovf_c), len(ovf),
                                p(e_cnt) if counted else None, p(ovf_cnt), min_depth, min_support, nr, chunk, p(R[0]), p(R[1]), p(R[2]), p(R[3]), p(depth), p(votes), p(step), p(iv), p(out))
    assert rc == 0, rc
    ni = int(out[0])
    st = np.asarray(w["st_off"]).astype(np.int64)
    got = {"n_graph_bases": n_flat, "n_steps": int(R[0][:nr].sum()), "n_steps_without_edge": int(out[1]),
           "rec_graph_bases": np.array([int(pre[st[r + 1]]) - int(pre[st[r]]) for r in range(nr)], np.uint64),
           "rec_steps": R[0][:nr], "rec_depth_sum": R[1][:nr]}
    for name, key in (("rec_depth_min", R[2][:nr]), ("rec_step_min", R[3][:nr])):
        none = key == np.uint64(0xFFFFFFFFFFFFFFFF)
        got[name] = np.where(none, NONE, key >> np.uint64(32)).astype(np.uint32)
        got[name + "_at"] = np.where(none, 0, key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    for j, k in enumerate(EM.IV_KEYS):
        got[k] = iv[j * max(n_flat, 1):j * max(n_flat, 1) + ni].copy()
    got.update(track_off=pre.astype(np.uint64), depth=depth[:n_flat], votes=votes[:n_flat], step=step[:n_flat])
    return got, (n_next, flags, ovf)


def check_unit(shim, m, w, chunks=(1 << 20, 64, 128)):
    u, g = m["u"], m["g"]
    for md, ms in thresholds(g, u.coverage):
        want = EM.evidence(g, u.coverage, w, m["sup"], md, ms, wm=m["wm"], node=m["node"])
        for chunk in (chunks if md else chunks[:1]):      # (the chunked replay where a depth threshold gives intervals to cut: at the build's coverage and above every node)
            got, _ = run_shim(shim, m, w, md, ms, chunk)
            assert EM.same(got, want, tracks=True) is None, (md, ms, chunk, EM.same(got, want, tracks=True))
    want = EM.evidence(g, u.coverage, w, None, u.coverage, 0, wm=m["wm"], node=m["node"])      # a unit without counters
    got, _ = run_shim(shim, m, w, u.coverage, 0, 1 << 20, counted=False)
    assert EM.same(got, want, tracks=True) is None and (got["step"] == NONE).all() and got["n_steps"] == 0
    return want


@pytest.mark.parametrize("name", list(UNITS))
def test_stretches_of_a_finish(shim, modelled, name):
    m = modelled(name)
    w = m["w"]
    assert len(w["rec_len"]) == m["pre"].count(b">") and len(w["id_first"]) > 0
    e = EM.evidence(m["g"], m["u"].coverage, w, m["sup"], 0, 0, wm=m["wm"], node=m["node"])
    assert e["n_steps_without_edge"] == 0, "a step of the walk that is no edge of the oracle's graph"
    assert (e["depth"] != NONE).all() and e["n_graph_bases"] == int(e["rec_graph_bases"].sum()) and len(e["iv_rec"]) == 0      # the walk only stands on nodes
    check_unit(shim, m, w)


@pytest.mark.parametrize("name", list(UNITS))
def test_hand_made_stretches(shim, modelled, name):
    m = modelled(name)
    check_unit(shim, m, m["hand"])


def test_hand_made_tables_reach_their_shapes(shim, modelled):
    """The hand-made tables hold what they are there for: a stretch across flat base 64, a depth tie inside a record, ids without a node, a step without an edge, and —
    on the overflow cases — a step whose counter lies on the overflow list, on a pair the list names twice."""
    seen = set()
    for name in [u.name for u in WALK_UNITS if u.overflow] + ["walk_kinds", "walk_hops", "walk_last_side", "seed201"]:
        m = modelled(name)
        w = m["hand"]
        first, base, rec, pre, join = flat_tables(w)
        e = EM.evidence(m["g"], m["u"].coverage, w, m["sup"], 0, 0, wm=m["wm"], node=m["node"])
        assert ((pre[:-1] < 64) & (pre[1:] > 64)).any()
        assert e["n_steps_without_edge"] >= 1
        assert e["rec_depth_min_at"][5] == 0 and e["depth"][int(pre[int(w["st_off"][5])])] >= e["rec_depth_min"][5]
        assert (np.bincount(rec, minlength=len(w["rec_len"]))[:5] == 1).all() and len(set(e["rec_depth_min"][2:5].tolist())) == 1      # three one-base records, equal minima
        if (e["depth"] == NONE).any():
            seen.add("no node")
        if (np.asarray(w["id_first"]) >= m["wm"]["n_pos"]).any():
            seen.add("side ids")
        got, (n_next, flags, ovf) = run_shim(shim, m, w, 0, 0, 1 << 20)
        if len(ovf):
            node, first_l, last_l, joined = m["node"], w["id_first"].tolist(), w["id_last"].tolist(), w["joined"].tolist()
            pairs, times = np.unique(ovf, axis=0, return_counts=True)
            twice = set(map(tuple, pairs[times > 1].tolist()))
            for i in range(1, len(first_l)):
                if joined[i] and (int(node[last_l[i - 1]]), int(node[first_l[i]])) in twice:
                    seen.add("overflow pair listed twice")
                    assert flags[int(node[last_l[i - 1]])] & EOVF
    assert seen >= {"no node", "side ids", "overflow pair listed twice"}, seen
