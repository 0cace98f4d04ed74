"""Passes 1, 2 and 3 of the node sweep (agx_k_node_sweep<1..3>, agx_kernels.hip), the lists that hand a tile from one pass to the next and the node pool's
per-region slices with the spill area behind them, on the units of tests/sweep_units.py: more tiles on each list than its pass has wavefronts (the strided
loops make a second and a third iteration on buckets that still hold the tile before), every bucket limit at its exact value and one beyond, a region that
takes ids from the spill area in a first build.  Every case against the oracle — node and edge tables field by field with the vote counters, the three output
files — and against the walk model (tests/walk_model.py: side_pk, tile_side and the side block with up to 63 x 1023 side ids in front of a lane); the passes'
statistics must equal what tests/sweep_units.py's model reads from the oracle's graph.  The unit with spilled ids also goes through everything downstream that
enters the node table through node_start: both unitig exports, the reprune, the edge support.  No CPU code runs this: the serial executor sweeps a tile with
one bucket and one counter (tests/test_sweep_cases.py, which makes the units and asserts that each reaches its arms).

Durations on an MI355X are in profiles/sweep_passes_gpu.txt."""
import os

import numpy as np
import pytest

import edge_support_model as ESM
import lean_units as LU
import sweep_units as SU
import unitig_model as UM
import unitig_region_model as URM
import walk_model as WM
from conftest import graph_mismatch
from hostsim import sim
from gpu_checks import check_counts, check_walk
from sweep_fixture import CASES, swept  # noqa: F401  (swept: the fixture)

import harness as H

pytestmark = pytest.mark.gpu

KEYS = ("initial", "pre", "extended")
SAME_STATS = ("n_pos", "n_hits", "n_nodes", "n_tiles", "n_tile_entries", "n_mid_tiles", "n_big_tiles", "n_edge_slow", "n_walk_ids", "n_special")


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def built_unit(agx, case, tmp, **kw):
    u = agx.Unit(k=LU.K, insert_variation=case.iv, coverage=case.coverage, keep_counts=True, **kw)
    u.load_files(tmp, 0)
    u.upload()
    u.build()
    return u


def look(u):
    """What a build left: the node and edge tables, the walk graph, and the statistics behind its download (which counts the walk ids)."""
    seen = {"graph": u.graph(), "walk": u.walk_graph(all_node=True)}
    seen["stats"] = u.stats()
    return seen


def check(case, o, ctx, seen, out):
    """One build against the oracle, the walk model and the sweep model."""
    assert graph_mismatch(o["graph"], seen["graph"]) is None
    st = dict(out["stats"])
    m = check_walk(o, [seen["walk"]], out, case.coverage)
    assert seen["stats"]["n_mid_tiles"] == ctx.n("mid"), (seen["stats"]["n_mid_tiles"], ctx.n("mid"))
    assert seen["stats"]["n_big_tiles"] == ctx.n("big"), (seen["stats"]["n_big_tiles"], ctx.n("big"))
    assert seen["stats"]["n_nodes"] == int(o["graph"]["n_nodes"])
    assert st["n_mid_tiles"] == ctx.n("mid") and st["n_big_tiles"] == ctx.n("big")
    if ctx.n("huge"):      # pass 3 is queued by a build that met such a tile: at least one attempt before the one that counts
        assert seen["stats"]["build_attempts"] >= 2
    return m


def run_case(agx, case, tmp, o, ctx):
    with built_unit(agx, case, tmp) as u:
        seen = look(u)
        out = u.finish()
        out["stats"] = u.stats()
    check(case, o, ctx, seen, out)
    return seen["stats"]


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.overflow])
def test_case_matches_oracle(agx, swept, name):
    case, tmp, o, s, ctx = swept(name)
    st = run_case(agx, case, tmp, o, ctx)
    print("%s: build_attempts %d, n_spilled %d, mid %d, big %d, huge (model) %d" % (name, st["build_attempts"], st["n_spilled"], st["n_mid_tiles"], st["n_big_tiles"], ctx.n("huge")))
    if name == "spill":
        d = int(ctx.demand[SU.SPILL_REGION])
        assert st["build_attempts"] == 1
        assert 0 < d - ctx.share <= st["n_spilled"] <= d, (st["n_spilled"], d)
    if name == "stride_big":      # spill_exhausted: the first build ran out of slices and spill area; the repeat's slices are cut to the demand and nothing spills
        assert st["build_attempts"] >= 2
        assert st["n_spilled"] == 0


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.overflow])
def test_case_beyond_the_last_bucket_is_refused(agx, swept, name):
    case, tmp, o, s, ctx = swept(name)
    SU.check_arms(case, ctx)
    with agx.Unit(k=LU.K, insert_variation=case.iv, coverage=case.coverage, keep_counts=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        with pytest.raises(agx.AgxError) as e:
            u.build()
    assert e.value.code == agx.AGX_E_OVERFLOW and str(SU.MAXV_HUGE) in e.value.msg


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.windows])
def test_case_swept_by_windows(agx, swept, name, monkeypatch):
    # pass 0 fills mid_list from three launches (tests/test_sweep_cases.py: each of these cases has deep tiles in two windows at least)
    case, tmp, o, s, ctx = swept(name)
    monkeypatch.setenv("AGX_UPLOAD_WINDOWS", "3")
    run_case(agx, case, tmp, o, ctx)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.rebuild])
def test_second_build_of_the_resident_unit(agx, swept, name):
    """The lists' counters and the spill counter start from zero again, the pool's layout and pass 3 stay as the first build left them: one attempt, the same
    tables, the same statistics."""
    case, tmp, o, s, ctx = swept(name)
    with built_unit(agx, case, tmp) as u:
        first = look(u)
        u.build()
        second = look(u)
        out = u.finish()
        out["stats"] = u.stats()
    m = check(case, o, ctx, first, out)
    assert graph_mismatch(first["graph"], second["graph"]) is None
    assert WM.mismatch(m, second["walk"]) is None
    for k in SAME_STATS:
        assert first["stats"][k] == second["stats"][k], k
    assert second["stats"]["build_attempts"] == 1
    if name == "spill":
        d = int(ctx.demand[SU.SPILL_REGION])
        assert first["stats"]["build_attempts"] == 1
        # which tiles reach the region's counter first decides how many ids spill: at least what the slice cannot hold (the tiles that fit are the first at the
        # counter); a spill counter that went on counting from the first build's would pass the demand
        assert 2 * (d - ctx.share) > d
        for st in (first["stats"], second["stats"]):
            assert d - ctx.share <= st["n_spilled"] <= d, (st["n_spilled"], d)
    else:
        assert first["stats"]["n_spilled"] == 0 and second["stats"]["n_spilled"] == 0


# ---- downstream of a node table with spilled ids -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spilled(agx, swept):
    """The spill case, built once, and everything downstream asked of that one unit: the exports, the edge support, then the reprune and its finish."""
    case, tmp, o, s, ctx = swept("spill")
    lo, hi = 90 * SU.TILE, 130 * SU.TILE
    got = {"lo": lo, "hi": hi}
    with built_unit(agx, case, tmp, edge_support=True) as u:
        got["stats"] = u.stats()
        got["graph"] = u.graph()
        got["gfa"] = u.gfa(0)
        got["unitigs"] = u.unitigs()
        got["whole_region"] = u.unitigs(region=(0, ctx.n_pos), min_coverage=case.coverage)
        got["region"] = {c: u.gfa(0, region=(lo, hi), min_coverage=c) for c in (0, 2)}
        got["support"] = u.edge_support()
        u.reprune(3)
        got["walk3"] = u.walk_graph(all_node=True)
        got["out3"] = u.finish()
        got["stats3"] = u.stats()
        got["support3"] = u.edge_support()
    return got


def test_spilled_unit_built_in_one_attempt(spilled, swept):
    case, tmp, o, s, ctx = swept("spill")
    assert spilled["stats"]["build_attempts"] == 1 and spilled["stats"]["n_spilled"] > 0
    assert graph_mismatch(o["graph"], spilled["graph"]) is None


def test_spilled_unit_whole_export(spilled, swept):
    case, tmp, o, s, ctx = swept("spill")
    assert spilled["gfa"] == UM.unit_gfa(o["graph"], case.coverage, UM.read_reference(tmp, 0), 0)
    assert spilled["gfa"].count(b"S\t") > 4 * 21
    a, b = spilled["unitigs"], spilled["whole_region"]
    assert sorted(a) == sorted(b) and all(np.array_equal(a[f], b[f]) for f in a if f != "seq") and a["seq"] == b["seq"]


@pytest.mark.parametrize("cov", [0, 2])
def test_spilled_unit_region_export(spilled, swept, cov):
    case, tmp, o, s, ctx = swept("spill")
    want = URM.region_gfa(o["graph"], spilled["lo"], spilled["hi"], cov, UM.read_reference(tmp, 0), 0)
    assert want.count(b"S\t") > 0
    assert spilled["region"][cov] == want


def test_spilled_unit_reprune(spilled, swept):
    case, tmp, o, s, ctx = swept("spill")
    m = WM.build(o["graph"], 3)
    assert WM.mismatch(m, spilled["walk3"]) is None
    want = H.run_oracle(tmp, 0, LU.K, case.iv, 3)
    for key in KEYS:
        assert spilled["out3"][key] == want[key], key
    assert (spilled["stats3"]["n_walk_ids"], spilled["stats3"]["n_special"]) == (m["n_ids"], m["n_special"])
    assert m["n_ids"] != WM.build(o["graph"], case.coverage)["n_ids"], "coverage 3 prunes nothing that coverage 1 keeps"


def test_spilled_unit_edge_support(spilled, swept):
    case, tmp, o, s, ctx = swept("spill")
    front = sim.run(tmp, 0, LU.K, case.iv, case.coverage, front=True)["front"]
    model = ESM.support(front, o["graph"], LU.K, case.iv)
    assert model["off_graph"] == 0
    check_counts(spilled["support"], spilled["graph"], model)
    check_counts(spilled["support3"], spilled["graph"], model)      # the counts do not depend on the prune
