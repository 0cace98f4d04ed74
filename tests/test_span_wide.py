"""tests/span_wide.py, the wide reference of the pair span (sorted endpoints, vectorised fragments and bases), against tests/span_model.py (loops), and the wide units of
tests/span_wide_units.py on the CPU.

The reference: on every unit of test_span_cases.UNITS and every hand-made front of span_units.window_fronts() the two agree field by field — fragments, pair_span at the
windows of test_span_cases.windows, and bases on the table of the unit's own finish, section 14's hand_made and span_tables.  The wide units (G, G + 1, G + 257 and 2 G + 65
hit records, G the records one round of the mark pass takes, from the library): the executor's front holds exactly that many records; the fragments from the construction,
from span_wide and from span_model are the same; the records behind G in the device's order hold a skipped hit, a fragment with runs and a simple fragment; the shapes the
units are there for occur; and unit_span equals the model's slice-increment loop (that loop is affordable at this size, the model's bases are not).
tests/test_gpu_span_wide.py runs the kernels on the same units.  Every comparison is integer equality."""
import ctypes
import os
import re

import numpy as np
import pytest

import span_model as SM
import span_units as SU
import span_wide as SW
import span_wide_units as WU
from hostsim import sim
from test_span_cases import UNITS, modelled, windows  # noqa: F401  (modelled: the module fixture)


def same_frags(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and tuple(a[2:4]) == tuple(b[2:4])


@pytest.mark.parametrize("name", list(UNITS))
def test_equals_the_model_on_the_units(modelled, name):
    m = modelled(name)
    front, n_pos = m["front"], m["n_pos"]
    frags = SW.fragments(front)
    assert same_frags(frags, m["frags"])
    for a, b in zip(SW.unit_span(front, frags), SM.unit_span(front, m["frags"])):
        assert np.array_equal(a, b)
    for win in windows(n_pos) + [None]:
        assert SM.same_span(SW.pair_span(front, win, frags), SM.pair_span(front, win, m["frags"])) is None, win
    for k, w in dict(m["tables"], own=m["w"]).items():
        got, want = SW.bases(front, m["side_xpos"], w, frags), SM.bases(front, m["side_xpos"], w, m["frags"])
        for i, (a, b) in enumerate(zip(got, want)):
            assert a == b, (k, "entry %d of the tuple" % i)
        assert SM.same(SM.walk_span(front, m["side_xpos"], w, 2, frags=frags, based=got), SM.walk_span(front, m["side_xpos"], w, 2, frags=m["frags"], based=want), tracks=True) is None, k


@pytest.mark.parametrize("name", list(SU.window_fronts()))
def test_equals_the_model_on_hand_made_fronts(name):
    front = SU.window_fronts()[name]
    n_pos = front["n_pos"]
    frags, want = SW.fragments(front), SM.fragments(front)
    assert same_frags(frags, want)
    for win in [None, (0, n_pos), (64, 64), (64, 65), (63, 65), (100, 140), (192, n_pos), (199, 200)]:
        assert SM.same_span(SW.pair_span(front, win, frags), SM.pair_span(front, win, want)) is None, win


def test_the_grid_comes_from_the_library():
    """G is AGX_SPAN_BLOCKS * 256 for every count of hits that fills the grid, the largest 32-bit count included (n_hits + 255 wrapped there and gave one workgroup)."""
    import aligngraph_amd as A
    with open(os.path.join(os.path.dirname(A.LIB_PATH), "csrc", "agx_kargs.h")) as h:
        blocks = int(re.search(r"#define\s+AGX_SPAN_BLOCKS\s+(\d+)u?", h.read()).group(1))
    g = WU.grid_hits()
    assert g == blocks * 256
    f = ctypes.CDLL(A.LIB_PATH).agx_span_partials
    f.argtypes, f.restype = [ctypes.c_uint32], ctypes.c_uint32
    for n, want in ((0, 1), (1, 1), (256, 1), (257, 2), (g - 256, blocks - 1), (g - 255, blocks), (g, blocks), (g + 1, blocks), (0xFFFFFF00, blocks), (0xFFFFFF01, blocks), (0xFFFFFFFF, blocks)):
        assert f(n) == 4 * want, (n, f(n))


@pytest.fixture(scope="module")
def wide(built, tmp_path_factory):
    """case -> dict(tmp, n_hits, g, rec: the construction's records in file order, front: the executor's in file order, order: the device's order of them): once per module"""
    g, sh, made = WU.grid_hits(), WU.shapes(), {}
    full = []

    def get(name):
        if name not in made:
            if not full:
                full.append(WU.write_full(str(tmp_path_factory.mktemp("wide_full")), g, sh))
            n_hits = WU.CASES[name](g)
            tmp = WU.write_case(full[0], str(tmp_path_factory.mktemp("wide")), n_hits, sh)
            rec = WU.records(n_hits, sh)
            front = sim.run(tmp, 0, WU.K, WU.IV, WU.COVERAGE, front=True)["front"]
            made[name] = {"tmp": tmp, "n_hits": n_hits, "g": g, "rec": rec, "front": front, "order": WU.device_order(rec["first_x"])}
        return made[name]
    return get


@pytest.mark.parametrize("name", list(WU.CASES))
def test_wide_units_hold_their_hit_records(wide, name):
    u = wide(name)
    want = {"G": u["g"], "G+1": u["g"] + 1, "G+257": u["g"] + 257, "2G+65": 2 * u["g"] + 65}[name]
    assert u["front"]["n_hits"] == len(u["front"]["dhit"]) == u["n_hits"] == want and u["front"]["n_pos"] == WU.N_POS


@pytest.mark.parametrize("name", list(WU.CASES))
def test_wide_fragments_three_ways(wide, name):
    u = wide(name)
    front, rec = u["front"], u["rec"]
    kept = rec["what"] != WU.SECOND
    built = (rec["f_lo"][kept], rec["f_hi"][kept], int(kept.sum()), 0)
    got = SW.fragments(front)
    assert same_frags(got, built), "span_wide.fragments against the construction"
    assert same_frags(SM.fragments(front), built), "span_model.fragments against the construction"
    f_lo, f_hi, at, is_kept, outside = SW.fragments_at(front)
    assert np.array_equal(at, np.nonzero(kept)[0]) and np.array_equal(is_kept, kept) and not outside.any()
    # the tile the device orders a hit by: the first aligned position of its left mate, as the construction says it
    assert np.array_equal(front["dhit"]["x_lo"][kept].astype(np.int64), rec["first_x"][kept])


@pytest.mark.parametrize("name", list(WU.CASES))
def test_wide_units_reach_the_later_rounds(wide, name):
    u = wide(name)
    front, rec, order, g = u["front"], u["rec"], u["order"], u["g"]
    # what the records are, read off the executor's front and laid out in the device's order
    a_lo, a_hi, b_lo, b_hi, kept, with_runs = SW.mates(front)
    what = np.where(~kept, WU.SECOND, np.where(with_runs, WU.RUNS, WU.SIMPLE))
    assert np.array_equal(what, rec["what"])
    behind = WU.assert_later_rounds(name, what[order], g)
    if name == "G+1":
        assert behind[WU.RUNS] == 1                                             # (the one hit of the second round has a deletion)
    # the shapes, anywhere in the unit
    n_pos = WU.N_POS
    assert int((kept & (b_lo < a_lo)).sum()) > 0, "no b mate left of its a mate"
    assert int((kept & (np.maximum(a_hi, b_hi) == n_pos - 1)).sum()) > 0, "no fragment that ends on the last position"
    runs = front["runs"]
    assert int((kept & with_runs).sum()) > 0 and len(runs) > 0
    gaps = runs["t"][1:].astype(np.int64) - runs["t"][:-1] - runs["n"][:-1], runs["q"][1:].astype(np.int64) - runs["q"][:-1] - runs["n"][:-1]
    assert ((gaps[0] == 5) & (gaps[1] == 0)).any() and ((gaps[0] == 0) & (gaps[1] == 3)).any(), "no deletion or no insertion among the runs"
    assert int((~kept).sum()) == int((rec["what"] == WU.SECOND).sum()) > 0


@pytest.mark.parametrize("name", list(WU.CASES))
def test_wide_unit_span_equals_the_model(wide, name):
    u = wide(name)
    front = u["front"]
    frags = SW.fragments(front)
    span, cross = SW.unit_span(front, frags)
    m_span, m_cross = SM.unit_span(front, frags)
    assert np.array_equal(span, m_span) and np.array_equal(cross, m_cross)
    assert int(cross[-1]) == 0 and int(span.max()) < 0xFFFFFFFF
    whole = SW.pair_span(front, None, frags)
    assert whole["n_fragments"] == whole["n_kept"] == u["n_hits"] - int((u["rec"]["what"] == WU.SECOND).sum()) and whole["n_outside"] == 0
