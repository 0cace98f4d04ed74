"""The lane functions of the pair span (csrc/agx_core.h: agx_span_fragment, agx_span_clamp, agx_span_pos, agx_span_step_kind, agx_span_jump_walk) on the CPU:
tests/span_shim.cpp runs them in a serial replay of mark / diff / scan / finish with its sub-window loop, and of gather / jump list / entries / count / scatter / flags /
runs with its chunk loop (the host's sort and merge is agx::span_jump_entries itself); tests/span_model.py — loops over fragments and bases, nothing of the engine —
says what must come out.  Every comparison is integer equality.

Units: every case of tests/walk_units.py, tests/edge_units.py and tests/lean_units.py and the generated seeds 201 and 203, each with the front of the serial executor
(file order), the stretches of a real finish through it, and hand-made stretch tables: span_tables() below on every unit, section 14's hand_made() on the walk units and
the seeds.  Hand-made fronts (tests/span_units.py) put mates exactly where a window's borders cut.  tests/test_gpu_span.py runs the kernels on the same units and
imports them from here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import harness as H
import path_model as PM
import span_model as SM
import span_units as SU
import walk_model as WM
from hostsim import sim
from test_edge_support_cases import EDGE_UNITS, LEAN_UNITS
from test_evidence_cases import SEED_UNITS, WALK_UNITS, executor_paths, flat_tables, hand_made

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIM_SRC = [os.path.join(HERE, "span_shim.cpp")]
NONE = SM.NONE
UNITS = {u.name: u for u in WALK_UNITS + EDGE_UNITS + LEAN_UNITS + SEED_UNITS}
WITH_NODES = {u.name for u in WALK_UNITS + SEED_UNITS}      # the units section 14's hand_made() tables are made for


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("span_shim") / "libspan_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so] + SHIM_SRC)
    L = ctypes.CDLL(so)
    front = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    L.agx_span_shim_pair.argtypes = front + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 3
    L.agx_span_shim_walk.argtypes = front + [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32] * 6 + [ctypes.c_void_p] * 9
    return L


def windows(n_pos):
    """(lo, hi) of the windows every unit is asked for: whole, empty, one position, [63, 65), mid-tile to mid-tile, the last partial tile"""
    c = lambda v: max(0, min(int(v), n_pos))
    last = n_pos - n_pos % 64 - (0 if n_pos % 64 else 64)
    return [(0, n_pos), (c(70), c(70)), (c(69), c(70)), (c(63), c(65)), (c(37), c(n_pos - 21)), (c(last), n_pos)]


def span_tables(n_pos, n_ids, side_xpos, frags):
    """Hand-made stretch tables for the jumps, the smallest shapes that can go wrong.  Record 0 (first, so that its flat bases are the table's): 64 bases and a joined
    stretch five positions on — the jump leaves flat base 63 and lands on flat base 64.  Then, around one fragment [f_lo, f_hi] of the unit: a jump f_lo -> f_hi (the
    fragment counts), a jump f_lo -> f_hi + 1 (it does not), the first jump once more in another record (one entry, two bases), first position -> last position,
    a joined pair on one position and a joined pair backwards (not forward), and — where the unit has side ids — a side id joined to a main id further on.
    Returns (table, the fragment)."""
    f_lo, f_hi = frags[0], frags[1]
    ok = np.nonzero((f_hi - f_lo >= 4) & (f_hi + 1 < n_pos))[0]
    if not len(ok) or n_pos < 80:      # (a unit whose every fragment reaches its last position, or too short for record 0: no table; the shapes test counts who has one)
        return None, None
    # the fragment whose relay is longest: most fragments end inside it, so that pairs(f_lo, f_hi + 1) tends to differ from the crossings in between
    i = int(ok[np.argmax((f_hi - f_lo)[ok])])
    a, b = int(f_lo[i]), int(f_hi[i])
    recs = [(80, [(0, 63, 0, 0), (68, 70, 64, 1)]),
            (4, [(a, a, 0, 0), (b, b, 1, 1)]),
            (4, [(a, a, 0, 0), (b + 1, b + 1, 1, 1)]),
            (9, [(a, a + 1, 2, 0), (b, b, 4, 1)]) if b > a + 2 else (4, [(a, a, 0, 0), (b, b, 1, 1)]),
            (4, [(a, a, 1, 0), (b, b, 2, 1)]),
            (2, [(0, 0, 0, 0), (n_pos - 1, n_pos - 1, 1, 1)]),
            (6, [(a, a, 0, 0), (a, a, 1, 1), (b, b, 2, 1), (a + 1, a + 2, 3, 1)]),
            (3, [])]
    if n_ids > n_pos:
        s = n_pos + (n_ids - n_pos) // 2
        p = int(side_xpos[s - n_pos])
        if p + 4 < n_pos:
            recs.append((8, [(s, s, 0, 0), (p + 3, p + 4, 1, 1)]))
        recs.append((70, [(n_pos, min(n_ids, n_pos + 66) - 1, 0, 0)]))      # consecutive side ids: their positions decide each step
    return PM.stretches(recs), (a, b)


@pytest.fixture(scope="module")
def modelled(built, tmp_path_factory):
    """name -> dict(u, tmp, front: the executor's in file order, frags, n_pos, n_ids, side_xpos: the walk model's, w: the executor's stretches, tables: name -> hand-made
    stretch table): made once per module"""
    made = {}

    def get(name):
        if name not in made:
            u = UNITS[name]
            tmp = u.write(str(tmp_path_factory.mktemp(name)))
            g = H.run_oracle(tmp, 0, u.k, u.iv, u.coverage, graph=True)["graph"]
            front = sim.run(tmp, 0, u.k, u.iv, u.coverage, front=True)["front"]
            w, _ = executor_paths(tmp, 0, u.k, u.iv, u.coverage)
            wm = WM.build(g, u.coverage)
            m = {"u": u, "tmp": tmp, "g": g, "wm": wm, "front": front, "frags": SM.fragments(front), "n_pos": int(front["n_pos"]), "n_ids": int(wm["n_ids"]),
                 "side_xpos": np.ascontiguousarray(wm["side_xpos"], np.uint32), "w": w}
            assert m["n_pos"] == int(wm["n_pos"])
            m["tables"] = {}
            jumps, around = span_tables(m["n_pos"], m["n_ids"], m["side_xpos"], m["frags"])
            if jumps is not None:
                m["tables"]["jumps"], m["around"] = jumps, around
            if name in WITH_NODES:
                m["tables"]["hand"] = hand_made(g, wm, PM.id_nodes(g, u.coverage, wm))
            made[name] = m
        return made[name]
    return get


def shuffled(front, seed=11):
    """The records in another order, as the device holds them (tile order): no number depends on it."""
    d = front["dhit"]
    return np.ascontiguousarray(d[np.random.RandomState(seed).permutation(len(d))]) if len(d) else np.zeros(1, SU.DHIT)


def run_pair(shim, front, lo, hi, sub=None, dhit=None):
    n_pos = int(front["n_pos"])
    d = np.ascontiguousarray(front["dhit"]) if dhit is None else dhit
    d = d if len(d) else np.zeros(1, SU.DHIT)
    runs = np.ascontiguousarray(front["runs"]) if len(front["runs"]) else np.zeros(1, SU.RUN)
    n = hi - lo
    span, cross, counts = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(4, np.uint64)
    rc = shim.agx_span_shim_pair(d.ctypes.data, len(front["dhit"]), runs.ctypes.data, len(front["runs"]), n_pos, lo, hi, sub or max(n, 1), span.ctypes.data, cross.ctypes.data,
                                 counts.ctypes.data)
    assert rc == 0, rc
    return {"pos_lo": lo, "pos_hi": hi, "n_fragments": int(counts[0]), "n_kept": int(counts[1]), "n_outside": int(counts[2]), "passes": int(counts[3]), "span": span[:n], "cross": cross[:n]}


def run_walk(shim, m, w, min_span, chunk=1 << 20, sub=None):
    front = m["front"]
    n_pos = m["n_pos"]
    d = shuffled(front)
    runs = np.ascontiguousarray(front["runs"]) if len(front["runs"]) else np.zeros(1, SU.RUN)
    side = m["side_xpos"] if len(m["side_xpos"]) else np.zeros(1, np.uint32)
    first, base, rec, pre, join = (np.ascontiguousarray(x) for x in flat_tables(w))
    n_st, n_flat, nr = len(first), int(pre[-1]), len(w["rec_len"])
    R = [np.zeros(max(nr, 1), np.uint64) for _ in range(4)]
    pos, span, step = (np.zeros(max(n_flat, 1), np.uint32) for _ in range(3))
    iv, out = np.zeros(5 * max(n_flat, 1), np.uint32), np.zeros(4, np.uint64)
    p = lambda a: a.ctypes.data
    rc = shim.agx_span_shim_walk(p(d), len(front["dhit"]), p(runs), len(front["runs"]), n_pos, p(side), m["n_ids"], p(first), p(base), p(rec), p(pre), p(join), n_st, n_flat,
                                 nr, min_span, chunk, sub or n_pos, p(R[0]), p(R[1]), p(R[2]), p(R[3]), p(pos), p(span), p(step), p(iv), p(out))
    assert rc == 0, rc
    ni = int(out[0])
    st = np.asarray(w["st_off"]).astype(np.int64)
    got = {"n_graph_bases": n_flat, "n_steps": int(R[0][:nr].sum()), "n_jump_steps": int(out[1]), "n_steps_not_forward": int(out[2]), "n_entries": int(out[3]),
           "rec_graph_bases": np.array([int(pre[st[r + 1]]) - int(pre[st[r]]) for r in range(nr)], np.uint64), "rec_steps": R[0][:nr], "rec_span_sum": R[1][:nr]}
    for name, key in (("rec_span_min", R[2][:nr]), ("rec_step_min", R[3][:nr])):
        none = key == np.uint64(0xFFFFFFFFFFFFFFFF)
        got[name] = np.where(none, NONE, key >> np.uint64(32)).astype(np.uint32)
        got[name + "_at"] = np.where(none, 0, key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    for j, k in enumerate(SM.IV_KEYS):
        got[k] = iv[j * max(n_flat, 1):j * max(n_flat, 1) + ni].copy()
    got.update(track_off=pre.astype(np.uint64), pos=pos[:n_flat], span=span[:n_flat], step=step[:n_flat])
    return got


def thresholds(m, based):
    """min_span every table is asked at: nothing, 1, the median span under the table, one above every span"""
    span = np.array(based[3], np.int64)
    return [0, 1, int(np.median(span)) if len(span) else 0, (int(span.max()) if len(span) else 0) + 1]


def check_table(shim, m, w, chunks=(1 << 20, 64, 128)):
    based = SM.bases(m["front"], m["side_xpos"], w, m["frags"])
    for t in thresholds(m, based):
        want = SM.walk_span(m["front"], m["side_xpos"], w, t, frags=m["frags"], based=based)
        for chunk in (chunks if t else chunks[:1]):
            got = run_walk(shim, m, w, t, chunk, sub=None if chunk > 128 else 100)      # (the chunked replays also make span and cross in sub-windows of 100)
            assert SM.same(got, want, tracks=True) is None, (t, chunk, SM.same(got, want, tracks=True))
    return based


@pytest.mark.parametrize("name", list(UNITS))
def test_pair_span_windows(shim, modelled, name):
    m = modelled(name)
    front, n_pos = m["front"], m["n_pos"]
    for lo, hi in windows(n_pos):
        want = SM.pair_span(front, (lo, hi), m["frags"])
        got = run_pair(shim, front, lo, hi, dhit=shuffled(front))
        assert SM.same_span(got, want) is None and got["passes"] == 1, (lo, hi, SM.same_span(got, want))
    whole = SM.pair_span(front, None, m["frags"])
    assert int(whole["cross"][-1]) == 0 and whole["n_outside"] == 0 and whole["n_fragments"] == whole["n_kept"]      # (the loaders make no hit beyond the unit)
    for sub in (64, 100):
        got = run_pair(shim, front, 0, n_pos, sub)
        assert SM.same_span(got, whole) is None and got["passes"] == -(-n_pos // sub), (sub, SM.same_span(got, whole))
        lo, hi = windows(n_pos)[4]
        assert SM.same_span(run_pair(shim, front, lo, hi, sub), SM.pair_span(front, (lo, hi), m["frags"])) is None, sub
    if name.startswith("seed"):
        assert whole["n_kept"] > 100 and int(whole["span"].max()) > 3 and len(front["runs"]) > 0      # mates with runs: the seeds' reads carry indels


@pytest.mark.parametrize("name", list(SU.window_fronts()))
def test_hand_made_fronts(shim, name):
    front = SU.window_fronts()[name]
    n_pos = front["n_pos"]
    frags = SM.fragments(front)
    for lo, hi in [(0, n_pos), (64, 64), (64, 65), (63, 65), (100, 140), (192, n_pos), (199, 200)]:
        want = SM.pair_span(front, (lo, hi), frags)
        for sub in (None, 64, 100, 7):
            got = run_pair(shim, front, lo, hi, sub)
            assert SM.same_span(got, want) is None, (lo, hi, sub, SM.same_span(got, want))
    f_lo, f_hi = frags[0].tolist(), frags[1].tolist()
    inside = lambda lo, hi: [(a, b) for a, b in zip(f_lo, f_hi) if a < hi and b >= lo]
    # every front holds the shape it is named for
    if name == "b_left_of_a":
        assert (40, 139) in zip(f_lo, f_hi) and int(front["dhit"][0]["b_t0"]) < int(front["dhit"][0]["a_t0"])
    elif name == "one_inside_the_other":
        assert (50, 129) in zip(f_lo, f_hi) and (64, 64) in zip(f_lo, f_hi) and SM.pair_span(front, (64, 65), frags)["cross"].tolist() == [1]
    elif name == "skipped":
        assert frags[2] == 1 and list(zip(f_lo, f_hi)) == [(63, 66)] and SM.pair_span(front, (20, 30), frags)["span"].sum() == 0
    elif name == "covers_the_window":
        assert (0, 199) in zip(f_lo, f_hi) and SM.pair_span(front, (100, 140), frags)["n_fragments"] == 2 and int(SM.pair_span(front, None, frags)["cross"][-1]) == 0
    elif name == "left_border_only":
        assert inside(64, 65) == [(40, 69)] and inside(100, 140) == [] and SM.pair_span(front, (64, 100), frags)["span"].tolist() == [1] * 6 + [0] * 30
    elif name == "right_border_only":
        assert inside(100, 140) == [(120, 159)] and SM.pair_span(front, (100, 140), frags)["cross"].tolist() == [0] * 20 + [1] * 20
    elif name == "over_the_end":
        assert list(zip(f_lo, f_hi)) == [(150, 199), (199, 199)] and (frags[2], frags[3]) == (3, 1)
        s = SM.pair_span(front, (192, 200), frags)
        assert s["span"].tolist() == [1] * 7 + [2] and s["cross"].tolist() == [1] * 7 + [0] and s["n_outside"] == 1
    elif name == "nothing":
        assert frags[2] == 0


@pytest.mark.parametrize("name", list(UNITS))
def test_stretches_of_a_finish(shim, modelled, name):
    m = modelled(name)
    w = m["w"]
    based = check_table(shim, m, w)
    assert based[7] == 0, "a step of the walk that is not forward"
    if len(w["id_first"]):
        assert len(based[0]) == int((np.asarray(w["id_last"]).astype(np.int64) - np.asarray(w["id_first"]) + 1).sum()) > 0


@pytest.mark.parametrize("name", list(UNITS))
def test_hand_made_stretches(shim, modelled, name):
    m = modelled(name)
    for w in m["tables"].values():
        check_table(shim, m, w)


def test_hand_made_tables_reach_their_shapes(shim, modelled):
    """The jump tables hold what they are there for — on every unit that has one the two jumps around a fragment's end, an entry two bases take, a jump nobody spans that
    is thin at min_span = 1, steps that are not forward and the jump out of flat base 63 — and somewhere a jump whose count differs from every crossing in between,
    side ids, and a stretch of consecutive side ids with jumps of its own."""
    seen, tried = set(), []
    for name in UNITS:
        m = modelled(name)
        if "jumps" not in m["tables"]:
            continue
        tried.append(name)
        w, (a, b) = m["tables"]["jumps"], m["around"]
        front, frags = m["front"], m["frags"]
        based = SM.bases(front, m["side_xpos"], w, frags)
        e = SM.walk_span(front, m["side_xpos"], w, 1, frags=frags, based=based)
        _, cross = SM.unit_span(front, frags)
        first, base, rec, pre, join = flat_tables(w)
        assert e["n_jump_steps"] >= 5 and e["n_steps_not_forward"] >= 2      # (more where side ids share a position)
        assert e["pos"][63] == 63 and e["pos"][64] == 68 and e["step"][63] == SM.pairs(frags, 63, 68) and pre[1] == 64      # the jump across the wave's border
        s1, s2, s3 = (int(pre[int(w["st_off"][r])]) for r in (1, 2, 3))
        assert e["step"][s1] == SM.pairs(frags, a, b) >= 1 and e["step"][s2] == SM.pairs(frags, a, b + 1) < e["step"][s1]      # y == f_hi counts the fragment, y == f_hi + 1 does not
        got = run_walk(shim, m, w, 1)
        assert got["n_entries"] < got["n_jump_steps"]                                                                         # two records take one (x, y)
        s5 = int(pre[int(w["st_off"][5])])
        assert e["pos"][s5] == 0 and e["pos"][s5 + 1] == m["n_pos"] - 1
        if e["step"][s5] == 0:
            seen.add("a jump nobody spans")
            assert ((e["iv_rec"] == 5) & (e["iv_first"] == 0)).any()                                                          # thin at min_span = 1, whatever its span
        if e["step"][s2] != int(cross[a:b + 1].min()) and e["step"][s2] != int(cross[a]):
            seen.add("differs from the crossings in between")
        if (np.asarray(w["id_first"]) >= m["n_pos"]).any():
            seen.add("side ids")
            last = len(w["rec_len"]) - 1
            sl = slice(int(pre[int(w["st_off"][last])]), int(pre[-1]))
            if (np.diff(e["pos"][sl].astype(np.int64)) != 1).any():
                seen.add("side ids that are not neighbours")
    assert len(tried) >= len(UNITS) // 2 and {"seed201", "seed203"} <= set(tried) and seen >= {"a jump nobody spans", "differs from the crossings in between", "side ids", "side ids that are not neighbours"}, (tried, seen)


def test_jump_entries_are_sorted_and_merged(shim, modelled):
    """The host's table: the shim refuses entries that are not strictly ascending by (x, y) (rc -6) and a scatter outside the flagged bases (rc -7); here the merged
    counts are also set against a direct count per base."""
    m = modelled("seed201")
    w = m["tables"]["jumps"]
    got = run_walk(shim, m, w, 0, 64)
    want = SM.walk_span(m["front"], m["side_xpos"], w, 0, frags=m["frags"])
    jump = np.nonzero((want["step"] != NONE) & (np.concatenate((np.diff(want["pos"].astype(np.int64)), [0])) != 1))[0]
    assert len(jump) >= 5 and np.array_equal(got["step"][jump], want["step"][jump])
