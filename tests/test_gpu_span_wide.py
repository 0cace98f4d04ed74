"""The pair span on the device past one grid of hit records (agx_k_span_mark, agx_k_sp_jumps: csrc/agx_span.hip) against tests/span_wide.py.

The two kernels stride over all hit records from at most AGX_SPAN_BLOCKS workgroups of 256 lanes; below G = AGX_SPAN_BLOCKS * 256 records `base += stride` never runs a
second time, and tests/test_gpu_span.py stays far below.  The units of tests/span_wide_units.py hold G, G + 1, G + 257 and 2 G + 65 hit records (G from the library; each
case asserts the engine's n_hits), and the records behind G in the device's order hold a skipped hit, a fragment with runs and a simple fragment.  Per unit one build, made
once per module, serves every check; the reference is span_wide on the front the device holds (Unit.front()), never another call of the engine, and every comparison is
integer equality: pair_span of the whole unit, of the windows of test_span_cases.windows and a second time; n_kept, n_fragments and n_outside against the construction;
sub-windows forced to 16 384 and to 100 positions (every sub-window one more pass of several rounds, and the passes must agree on their counts); walk_span with tracks on
the table of the unit's own finish, on test_span_cases.span_tables made for the unit and on a table of jumps across the unit's last tile — where the fragments behind G
lie, so that an entry of agx_k_sp_jumps is counted in a later round (asserted, and named, in every case that has a record behind G) — at the four thresholds
of test_span_cases.thresholds and once more in base chunks of 128 with sub-windows of 100; the finish before and after; device_bytes and hbm_needed().  A failure names the case, the call, the first field and index that differ and how many
fragments of records behind G cover that position: that number says whether a later round went missing."""
import os

import numpy as np
import pytest

import harness as H
import path_model as PM
import span_model as SM
import span_wide as SW
import span_wide_units as WU
import walk_model as WM
from test_span_cases import span_tables, thresholds, windows

pytestmark = pytest.mark.gpu

NAMES = list(WU.CASES)
LATE_X = WU.TOP_TILE * WU.TILE + 20      # a position of the last tile a left mate can begin in: every shape of that tile has begun by here or begins within two positions


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


@pytest.fixture(scope="module")
def prepared(built, tmp_path_factory):
    """case -> dict(tmp, n_hits, g, rec: the construction's records in file order, side_xpos, n_ids: the walk model's over the oracle's graph).  The CPU side of all four
    units, made when the module's first test is set up."""
    g, sh = WU.grid_hits(), WU.shapes()
    full = WU.write_full(str(tmp_path_factory.mktemp("wide_full")), g, sh)
    out = {}
    for name in NAMES:
        n_hits = WU.CASES[name](g)
        tmp = WU.write_case(full, str(tmp_path_factory.mktemp("wide")), n_hits, sh)
        wm = WM.build(H.run_oracle(tmp, 0, WU.K, WU.IV, WU.COVERAGE, graph=True)["graph"], WU.COVERAGE)
        assert int(wm["n_pos"]) == WU.N_POS
        out[name] = {"tmp": tmp, "n_hits": n_hits, "g": g, "rec": WU.records(n_hits, sh), "side_xpos": np.ascontiguousarray(wm["side_xpos"], np.uint32), "n_ids": int(wm["n_ids"])}
    return out


def late_table(n_pos):
    """Jumps across the unit's last tile: LATE_X -> the last position, LATE_X -> 40 positions on, and one from in front of the tile into it."""
    return PM.stretches([(4, [(LATE_X, LATE_X, 0, 0), (n_pos - 1, n_pos - 1, 1, 1)]), (4, [(LATE_X, LATE_X, 0, 0), (LATE_X + 40, LATE_X + 40, 1, 1)]),
                         (6, [(LATE_X - 30, LATE_X - 30, 0, 0), (LATE_X + 5, LATE_X + 6, 1, 1)])])


def forced(env, call, *a, **kw):
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return call(*a, **kw)
    finally:
        for k in env:
            del os.environ[k]


def run_engine(agx, p):
    """One build of the unit; everything the tests look at, collected before the unit goes."""
    n_pos, out = WU.N_POS, {}
    with agx.Unit(k=WU.K, insert_variation=WU.IV, coverage=WU.COVERAGE, keep_counts=True, keep_paths=True) as e:
        e.load_files(p["tmp"], 0)
        e.upload()
        e.build()
        front = e.front()
        out["front"] = {k: front[k] for k in ("n_pos", "n_hits", "dhit", "runs", "perm")}
        out["need"] = e.hbm_needed()
        out["fin"] = e.finish()
        w = out["w"] = e.walk_paths()
        e.unitigs()
        out["stats0"] = e.stats()
        out["pair"] = {win: e.pair_span(win) for win in windows(n_pos)}
        out["whole"] = e.pair_span()
        out["again"] = e.pair_span()
        out["sub"] = {c: forced({"AGX_SPAN_CHUNK": c}, e.pair_span) for c in (16384, 100)}
        out["stats1"] = e.stats()
        # the reference, from the front the device holds
        f = out["front"]
        f_lo, f_hi, at, kept, outside = SW.fragments_at(f)
        frags = out["frags"] = (f_lo, f_hi, int(kept.sum()), int(outside.sum()))
        out["at"] = at
        out["spans"] = SW.unit_span(f, frags)
        jumps, out["around"] = span_tables(n_pos, p["n_ids"], p["side_xpos"], frags)
        out["tables"] = {"own": w, "jumps": jumps, "late": late_table(n_pos)}
        out["based"] = {k: SW.bases(f, p["side_xpos"], t, frags) for k, t in out["tables"].items()}
        out["ts"] = {k: thresholds(None, b) for k, b in out["based"].items()}
        out["walk"] = {(k, t): e.walk_span(tab, t, tracks=True) for k, tab in out["tables"].items() for t in out["ts"][k]}
        out["chunks"] = {k: forced({"AGX_SPAN_BASE_CHUNK": 128, "AGX_SPAN_CHUNK": 100}, e.walk_span, tab, out["ts"][k][2], tracks=True) for k, tab in out["tables"].items()}
        out["need2"] = e.hbm_needed()
        out["stats2"] = e.stats()
        out["fin_again"] = e.finish()
    return out


@pytest.fixture(scope="module")
def engine_of(agx, prepared):
    made = {}

    def get(name):
        if name not in made:
            made[name] = run_engine(agx, prepared[name])
        return made[name]
    return get


def late_over(e, g, x, y=None):
    """The fragments of records at index >= g (the device's order) that cover position x (and reach y)."""
    f_lo, f_hi = e["frags"][:2]
    late = e["at"] >= g
    return int((late & (f_lo <= x) & (f_hi >= (x if y is None else y))).sum())


def first_diff(got, want):
    a, b = np.asarray(got).astype(np.int64).reshape(-1), np.asarray(want).astype(np.int64).reshape(-1)
    if len(a) != len(b):
        return min(len(a), len(b))
    return int(np.nonzero(a != b)[0][0])


def assert_span(name, call, got, want, e, g):
    d = SM.same_span(got, want)
    if d is None:
        return
    if d in ("span", "cross"):
        i = first_diff(got[d], want[d])
        x = int(want["pos_lo"]) + i
        raise AssertionError("case %s, %s: %s differs first at index %d (position %d): got %s, want %s; %d fragments of records behind G = %d cover that position" %
                             (name, call, d, i, x, np.asarray(got[d]).tolist()[i:i + 1], np.asarray(want[d]).tolist()[i:i + 1], late_over(e, g, x), g))
    raise AssertionError("case %s, %s: %s is %d, want %d; %d fragments belong to records behind G = %d" % (name, call, d, int(got[d]), int(want[d]), int((e["at"] >= g).sum()), g))


def assert_walk(name, call, got, want, e, g):
    d = SM.same(got, want, tracks=True)
    if d is None:
        return
    if d in SM.TOTALS:
        raise AssertionError("case %s, %s: %s is %d, want %d" % (name, call, d, int(got[d]), int(want[d])))
    i = first_diff(got[d], want[d])
    x = int(want["pos"][i]) if d in SM.TRACK_KEYS[1:] and i < len(want["pos"]) else None
    raise AssertionError("case %s, %s: %s differs first at index %d%s: got %s, want %s; %s" %
                         (name, call, d, i, "" if x is None else " (position %d)" % x, np.asarray(got[d]).tolist()[i:i + 1], np.asarray(want[d]).tolist()[i:i + 1],
                          "%d fragments belong to records behind G = %d" % (int((e["at"] >= g).sum()), g) if x is None else
                          "%d fragments of records behind G = %d cover that position" % (late_over(e, g, x), g)))


def wanted_span(e, win):
    return SW.pair_span(e["front"], win, e["frags"], e["spans"])


@pytest.mark.parametrize("name", NAMES)
def test_hit_records_and_later_rounds(engine_of, prepared, name):
    p, e = prepared[name], engine_of(name)
    g, rec, f = p["g"], p["rec"], e["front"]
    want = {"G": g, "G+1": g + 1, "G+257": g + 257, "2G+65": 2 * g + 65}[name]
    assert e["stats0"]["n_hits"] == f["n_hits"] == len(f["dhit"]) == p["n_hits"] == want and e["stats0"]["n_pos"] == f["n_pos"] == WU.N_POS
    assert np.array_equal(f["perm"].astype(np.int64), WU.device_order(rec["first_x"])), "the device's order is not the first tiles' with file order inside a tile"
    a_lo, a_hi, b_lo, b_hi, kept, with_runs = SW.mates(f)
    what = np.where(~kept, WU.SECOND, np.where(with_runs, WU.RUNS, WU.SIMPLE))
    assert np.array_equal(what, rec["what"][f["perm"]])
    WU.assert_later_rounds(name, what, g)
    # the fragments the device's records give are the construction's, record by record
    in_file = f["perm"][e["at"]]
    assert np.array_equal(e["frags"][0], rec["f_lo"][in_file]) and np.array_equal(e["frags"][1], rec["f_hi"][in_file])
    assert int((kept & (b_lo < a_lo)).sum()) > 0 and int((e["frags"][1] == WU.N_POS - 1).sum()) > 0


@pytest.mark.parametrize("name", NAMES)
def test_pair_span(engine_of, prepared, name):
    p, e = prepared[name], engine_of(name)
    assert_span(name, "pair_span()", e["whole"], wanted_span(e, None), e, p["g"])
    for win, got in e["pair"].items():
        assert_span(name, "pair_span(%s)" % (win,), got, wanted_span(e, win), e, p["g"])
    assert_span(name, "a second pair_span()", e["again"], wanted_span(e, None), e, p["g"])
    assert int(e["whole"]["cross"][-1]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_counts_against_the_construction(engine_of, prepared, name):
    p, e = prepared[name], engine_of(name)
    kept = int((p["rec"]["what"] != WU.SECOND).sum())
    for call, got in [("pair_span()", e["whole"]), ("a second pair_span()", e["again"])] + [("pair_span() in sub-windows of %d" % c, s) for c, s in e["sub"].items()]:
        assert (got["n_kept"], got["n_fragments"], got["n_outside"]) == (kept, kept, 0), (name, call, got["n_kept"], got["n_fragments"], got["n_outside"], kept)
    lo, hi = windows(WU.N_POS)[4]
    meets = int(((p["rec"]["f_lo"] < hi) & (p["rec"]["f_hi"] >= lo) & (p["rec"]["what"] != WU.SECOND)).sum())
    got = e["pair"][(lo, hi)]
    assert (got["n_kept"], got["n_fragments"], got["n_outside"]) == (kept, meets, 0), (name, (lo, hi))


@pytest.mark.parametrize("name", NAMES)
def test_forced_sub_windows(engine_of, prepared, name):
    p, e = prepared[name], engine_of(name)
    for c, got in e["sub"].items():
        assert_span(name, "pair_span() in sub-windows of %d" % c, got, wanted_span(e, None), e, p["g"])


@pytest.mark.parametrize("name", NAMES)
def test_walk_span_tables(engine_of, prepared, name):
    p, e = prepared[name], engine_of(name)
    f, g = e["front"], p["g"]
    for k, tab in e["tables"].items():
        for t in e["ts"][k]:
            want = SM.walk_span(f, p["side_xpos"], tab, t, frags=e["frags"], based=e["based"][k])
            assert_walk(name, "walk_span(%s, %d, tracks=True)" % (k, t), e["walk"][(k, t)], want, e, g)
    own = e["walk"][("own", 0)]
    assert own["n_steps_not_forward"] == 0 and len(own["iv_rec"]) == 0 and own["n_graph_bases"] > 0
    late = e["walk"][("late", 0)]
    assert late["n_jump_steps"] == 3 and late["pos"].tolist() == [LATE_X, WU.N_POS - 1, LATE_X, LATE_X + 40, LATE_X - 30, LATE_X + 5, LATE_X + 6]
    if p["n_hits"] > g:      # an entry agx_k_sp_jumps counts in a later round: the jump LATE_X -> LATE_X + 40 is spanned by a fragment of a record behind G
        n = late_over(e, g, LATE_X, LATE_X + 40)
        assert n >= 1, "case %s: no fragment of a record behind G = %d spans the jump %d -> %d of table late" % (name, g, LATE_X, LATE_X + 40)
        assert int(late["step"][2]) == SW.pairs(e["frags"], LATE_X, LATE_X + 40) >= n, \
            "case %s: the jump %d -> %d of table late, spanned by %d fragments of records behind G = %d, has step %d" % (name, LATE_X, LATE_X + 40, n, g, int(late["step"][2]))


@pytest.mark.parametrize("name", NAMES)
def test_forced_base_chunks(engine_of, prepared, name):
    p, e = prepared[name], engine_of(name)
    for k, tab in e["tables"].items():
        t = e["ts"][k][2]
        want = SM.walk_span(e["front"], p["side_xpos"], tab, t, frags=e["frags"], based=e["based"][k])
        assert_walk(name, "walk_span(%s, %d, tracks=True) in base chunks of 128, sub-windows of 100" % (k, t), e["chunks"][k], want, e, p["g"])


@pytest.mark.parametrize("name", NAMES)
def test_disturbs_nothing(engine_of, prepared, name):
    e = engine_of(name)
    assert e["fin_again"] == e["fin"]                                                    # the finish behind it all, byte for byte
    assert e["stats0"]["device_bytes"] == e["stats1"]["device_bytes"] == e["stats2"]["device_bytes"] and e["need"] == e["need2"]      # sampled after one export
