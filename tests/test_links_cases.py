"""The lane functions of the mate links (csrc/agx_core.h: agx_links_class, agx_links_key, agx_links_hash, agx_links_insert) on the CPU: tests/links_shim.cpp runs them in
a serial replay of init / own / shadow / pass / flag / scan / emit under the host's own range-halving loop (agx::links_plan, csrc/agx_host.h); tests/links_model.py —
loops over bases and fragments and a dict, nothing of the engine — says what must come out.  Every comparison is integer equality, and the identity over the totals is
asserted in every case.

Units: those of tests/test_span_cases.py (every case of tests/walk_units.py, tests/edge_units.py and tests/lean_units.py, the seeds 201 and 203) and the hand-made fronts of
tests/span_units.py.  Tables: the stretches of a real finish through the serial executor, section 16's span_tables, and tests/links_units.py (records interleaved by
position, every base a record, records stacked over the same positions, no record, one record).  Slot counts: the natural size, exactly the number of distinct keys (every
key still finds a slot in one pass), one fewer (the range is split, the answer stays), and 2 slots where a record has three links (refused).
tests/test_gpu_links.py runs the kernels on the same units and imports them from here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import links_model as LM
import links_units as LU
import path_model as PM
import span_model as SM
import span_units as SU
from test_evidence_cases import flat_tables
from test_span_cases import UNITS, modelled, shuffled  # noqa: F401  (modelled: the module fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = [os.path.join(HERE, "links_shim.cpp")]
NONE = LM.NONE
UNSUPPORTED = -1


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("links_shim") / "liblinks_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so] + SHIM_SRC)
    L = ctypes.CDLL(so)
    L.agx_links_shim.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5 + \
                                [ctypes.c_uint32] * 5 + [ctypes.c_void_p] * 6 + [ctypes.c_uint32]
    L.agx_links_shim_hash.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.agx_links_shim_hash.restype = ctypes.c_uint32
    return L


def pow2_at_least(v):
    n = 2
    while n < v:
        n *= 2
    return n


def natural_slots(n_hits, n_recs):
    """the engine's own choice where the scratch has room: twice the keys there can be at most"""
    return pow2_at_least(2 * min(n_hits, n_recs * max(n_recs - 1, 0)))


def hit_of_fragment(m):
    """the hit behind every fragment of the unit, in the order of span_model.fragments (made once per unit)"""
    if "hit_of_frag" not in m:
        front = m["front"]
        m["hit_of_frag"] = [i for i in range(len(front["dhit"])) if len(SM.fragments(dict(front, dhit=front["dhit"][i:i + 1]))[0])]
        assert len(m["hit_of_frag"]) == len(m["frags"][0])
    return m["hit_of_frag"]


def prefix_front(m, w, n_keys):
    """The shortest prefix of the unit's hits (file order) whose links under w have exactly n_keys distinct keys: a table of n_keys slots — a slot count is a power of
    two — is then full to the last slot."""
    own = LM.owners(m["n_pos"], m["side_xpos"], w)[0]
    keys = set()
    for j, (lo, hi) in enumerate(zip(m["frags"][0].tolist(), m["frags"][1].tolist())):
        a, b = own[lo], own[hi]
        if a != NONE and b != NONE and a != b:
            keys.add((a, b))
            if len(keys) == n_keys:
                return dict(m["front"], dhit=np.ascontiguousarray(m["front"]["dhit"][:hit_of_fragment(m)[j] + 1]))
    raise AssertionError("the table has fewer keys")


def forced_slots(n_keys):
    """the largest power of two of keys a table with n_keys distinct links can be cut to (None: fewer than two keys)"""
    return None if n_keys < 2 else 1 << (n_keys.bit_length() - 1)


def tables_of(m):
    """name -> stretch table of a modelled unit: its finish's, section 16's, tests/links_units.py's"""
    t = dict(m["tables"], own=m["w"])
    t.update(LU.links_tables(m["n_pos"]))
    return t


def run_links(shim, front, n_ids, side_xpos, w, min_pairs=1, slots=None, dhit=None):
    n_pos = int(front["n_pos"])
    d = np.ascontiguousarray(front["dhit"]) if dhit is None else dhit
    d = d if len(d) else np.zeros(1, SU.DHIT)
    runs = np.ascontiguousarray(front["runs"]) if len(front["runs"]) else np.zeros(1, SU.RUN)
    side = np.ascontiguousarray(side_xpos, np.uint32) if len(side_xpos) else np.zeros(1, np.uint32)
    first, base, rec, pre, join = (np.ascontiguousarray(x) if len(x) else np.zeros(1, x.dtype) for x in flat_tables(w))
    n_st, nr = len(w["id_first"]), len(w["rec_len"])
    n_flat = int(flat_tables(w)[3][-1])
    nh = len(front["dhit"])
    cap = max(nh, 1)
    totals, R, own = np.zeros(13, np.uint64), np.zeros(5 * max(nr, 1), np.uint32), np.zeros(max(n_pos, 1), np.uint32)
    l_key, l_len, l_num = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(5 * cap, np.uint32)
    p = lambda a: a.ctypes.data
    slots = slots or natural_slots(nh, nr)
    rc = shim.agx_links_shim(p(d), nh, p(runs), len(front["runs"]), n_pos, p(side), n_ids, p(first), p(base), p(rec), p(pre), p(join), n_st, n_flat, nr, min_pairs, slots,
                             p(totals), p(R), p(own), p(l_key), p(l_len), p(l_num), cap)
    if rc == UNSUPPORTED:
        return {"rc": rc, "stuck": int(totals[9])}
    assert rc == 0, rc
    t = [int(v) for v in totals]
    nl = t[10]
    got = {"rc": 0, "n_kept": t[0], "n_outside": t[1], "n_fragments": t[0] - t[1], "n_unowned": t[2], "n_inside": t[3], "n_open": t[4], "n_link_pairs": t[5], "n_owned": t[6],
           "n_shadowed": t[7], "n_links_all": t[8], "n_passes": t[9], "single_record_passes": t[11], "probes": t[12], "n_slots": slots, "own": own[:n_pos]}
    for j, k in enumerate(LM.REC_KEYS):
        got[k] = R[j * nr:(j + 1) * nr].copy()
    got.update(a=(l_key[:nl] >> np.uint64(32)).astype(np.uint32), b=(l_key[:nl] & np.uint64(0xFFFFFFFF)).astype(np.uint32), len_sum=l_len[:nl].copy())
    for j, k in enumerate(("n_pairs", "lo_min", "lo_max", "hi_min", "hi_max")):
        got[k] = l_num[j * cap:j * cap + nl].copy()
    return got


def thresholds(want):
    """min_pairs every table is asked at: 0, 1, 2 and one above every count"""
    return [0, 1, 2, (int(want["n_pairs"].max()) if len(want["n_pairs"]) else 0) + 1]


def check_table(shim, m, w, seen=None):
    """One table of one unit at every threshold and every slot count it lends itself to; returns the model's answer at min_pairs 1."""
    front, frags, n_pos, n_ids, side = m["front"], m["frags"], m["n_pos"], m["n_ids"], m["side_xpos"]
    all_links = LM.mate_links(frags, n_pos, side, w, 1)
    assert LM.identity(all_links)
    d = shuffled(front)
    for t in thresholds(all_links):
        want = LM.mate_links(frags, n_pos, side, w, t)
        got = run_links(shim, front, n_ids, side, w, t, dhit=d)
        assert LM.same(got, want) is None and LM.identity(got) and got["n_passes"] == 1, (t, LM.same(got, want))
    own = np.array(LM.owners(n_pos, side, w)[0], np.uint32)
    assert np.array_equal(run_links(shim, front, n_ids, side, w)["own"], own)
    exact = forced_slots(all_links["n_links_all"])
    if exact:      # exactly as many slots as keys, and one fewer, on the prefix of the hits that has a power of two of keys
        front = prefix_front(m, w, exact)
        frags, d = SM.fragments(front), shuffled(front, 5)
        full = LM.mate_links(frags, n_pos, side, w, 1)
        assert full["n_links_all"] == exact
        got = run_links(shim, front, n_ids, side, w, 1, slots=exact, dhit=d)
        assert LM.same(got, full) is None and got["n_passes"] == 1 and LM.identity(got), ("exact", exact, LM.same(got, full))
        if seen is not None and got["probes"] > 0:
            seen.add("two keys with one home slot")
    if exact and exact >= 4:
        fewer = exact // 2
        for t in (1, 2):
            got = run_links(shim, front, n_ids, side, w, t, slots=fewer, dhit=d)
            if got["rc"] == UNSUPPORTED:      # (one record alone has more links than slots: the refusal, with the record)
                out = np.bincount(full["a"], minlength=len(w["rec_len"]))
                assert out[got["stuck"]] > fewer
                if seen is not None:
                    seen.add("refused")
                continue
            want = LM.mate_links(frags, n_pos, side, w, t)
            assert LM.same(got, want) is None and got["n_passes"] >= 3 and LM.identity(got), ("fewer", fewer, t, LM.same(got, want))
            if seen is not None:
                seen.add("split")
                if got["single_record_passes"]:
                    seen.add("a split down to one record")
    if seen is not None:
        if (all_links["lo_min"] != all_links["lo_max"]).any():
            seen.add("lo_min != lo_max")
        if all_links["n_shadowed"]:
            seen.add("shadowed")
        a, b = all_links["a"].tolist(), all_links["b"].tolist()
        if set(zip(a, b)) & set(zip(b, a)):
            seen.add("both directions")
    return all_links


SEEN = set()


@pytest.mark.parametrize("name", list(UNITS))
def test_units_and_tables(shim, modelled, name):
    m = modelled(name)
    for k, w in tables_of(m).items():
        l = check_table(shim, m, w, SEEN)
        if k in ("empty", "one_record"):
            assert l["n_links_all"] == 0 and l["n_link_pairs"] == 0
        if k == "empty":
            assert l["n_unowned"] == l["n_fragments"] and l["n_owned"] == 0
        if k == "one_record":
            assert l["n_inside"] == l["n_fragments"] and l["n_owned"] == m["n_pos"]
        if k == "stacked":
            q = m["n_pos"] // 4
            assert l["n_shadowed"] == 2 * q and l["n_owned"] == m["n_pos"] and l["rec_inside"][2] == 0


@pytest.mark.parametrize("name", list(SU.window_fronts()))
def test_hand_made_fronts(shim, name):
    front = SU.window_fronts()[name]
    n_pos = front["n_pos"]
    m = {"front": front, "frags": SM.fragments(front), "n_pos": n_pos, "n_ids": n_pos, "side_xpos": np.zeros(0, np.uint32)}
    for k, w in LU.links_tables(n_pos).items():
        l = check_table(shim, m, w)
        if name == "skipped":
            assert l["n_kept"] == 1 and l["n_fragments"] == 1
        if name == "over_the_end":
            assert l["n_outside"] == 1 and l["n_fragments"] == 2
        if name == "nothing":
            assert l["n_fragments"] == 0 and l["n_links_all"] == 0


def hand_case():
    """four records of six positions ten apart and five kept hits: record 0 has three links out, record 1 two"""
    front = SU.hand_front(40, [dict(a=2, b=10, len=2), dict(a=3, b=20, len=2), dict(a=2, b=30, len=2), dict(a=12, b=31, len=2), dict(a=21, b=4, len=1, skip=True), dict(a=11, b=22, len=3)])
    w = PM.stretches([(6, [(0, 5, 0, 0)]), (6, [(10, 15, 0, 0)]), (6, [(20, 25, 0, 0)]), (6, [(30, 35, 0, 0)])])
    return {"front": front, "frags": SM.fragments(front), "n_pos": 40, "n_ids": 40, "side_xpos": np.zeros(0, np.uint32)}, w


def test_two_slots_and_a_record_with_three_links(shim):
    """Record 0 has the links (0, 1), (0, 2) and (0, 3): they never fit 2 slots, however the records are halved; with 4 slots one pass holds them beside (1, 3) and
    (1, 2) only after a split."""
    m, w = hand_case()
    want = LM.mate_links(m["frags"], 40, m["side_xpos"], w, 1)
    assert list(zip(want["a"].tolist(), want["b"].tolist())) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)] and want["n_kept"] == 5
    got = run_links(shim, m["front"], 40, m["side_xpos"], w, 1, slots=2)
    assert got == {"rc": UNSUPPORTED, "stuck": 0}
    got = run_links(shim, m["front"], 40, m["side_xpos"], w, 1, slots=4)
    # five keys: records [0, 4) overflow, [0, 2) still hold all five, [0, 1) holds three, [1, 2) two, [2, 4) none
    assert LM.same(got, want) is None and got["n_passes"] == 5 and got["n_links_all"] == 5 and got["single_record_passes"] == 2
    assert LM.same(run_links(shim, m["front"], 40, m["side_xpos"], w, 1, slots=8), want) is None


def test_the_cases_reach_their_shapes(shim, modelled):
    """Somewhere among the units and tables: two keys with the same home slot, a link with lo_min != lo_max, a split that ends in ranges of one record, links in both
    directions, shadowed bases."""
    seen = set()
    for name in ("seed201", "seed203", "walk_kinds"):
        m = modelled(name)
        for w in tables_of(m).values():
            check_table(shim, m, w, seen)
    # two keys of one table with one home slot, said by the hash itself
    m = modelled("seed201")
    l = LM.mate_links(m["frags"], m["n_pos"], m["side_xpos"], LU.links_tables(m["n_pos"])["every_base"], 1)
    keys = (l["a"].astype(np.uint64) << np.uint64(32)) | l["b"].astype(np.uint64)
    slots = pow2_at_least(len(keys))      # (the smallest table that holds them all)
    homes = [shim.agx_links_shim_hash(int(k), slots.bit_length() - 1) for k in keys.tolist()]
    assert len(keys) > 50 and len(set(homes)) < len(homes) and max(homes) < slots
    assert seen >= {"two keys with one home slot", "lo_min != lo_max", "split", "a split down to one record", "both directions", "shadowed"}, seen
