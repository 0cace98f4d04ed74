"""The compatibility windows at their edges on the device: the units of tests/window_units.py (clause C, clause B and clause A on the node side and the edge side, each
difference at win - 1, win, win + 1 on both sides) through the HIP engine.  Per case one build serves the checks: agx_unit_graph against the oracle field by field (a
failure names the case, the position, the variant and both keys), finish() against the md5s the reference itself wrote (tests/golden/hand_units_reference.json),
edge_support() against tests/edge_support_model.py, a second build of the resident unit, and the outputs after a reprune to every coverage the case names.  Then the
same under AGX_UPLOAD_WINDOWS=3 and under AGX_TEST_SMALL_CAPS=1.  Every comparison is exact.  tests/test_window_cases.py runs the same cases through the serial
executor; pass 0's own arithmetic for the windows (agx_sweep_tile_lean) has no CPU twin and is held here alone."""
import os

import pytest

import edge_support_model as ESM
import harness as H
import lean_units as LU
import window_units as WU
from golden import make_hand_units_reference as R
from gpu_checks import check_counts
from hostsim import sim

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in WU.cases()}
TABLE = R.load()


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


@pytest.fixture(scope="module")
def unit_of(built, tmp_path_factory):
    """Writes a case's unit, checks on the oracle and the executor that it sits on its edges, and models its edge support, once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = case.write(str(tmp_path_factory.mktemp(name)))
            assert R.inputs_md5(tmp) == TABLE["window:" + name]["inputs_md5"], "the unit's files changed: regenerate tests/golden/hand_units_reference.json"
            o = H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True)
            s = sim.run(tmp, 0, LU.K, case.iv, case.coverage, graph=True, edges=True, records=True, front=True)
            WU.check(case, o, s)
            made[name] = (case, tmp, o, ESM.support(s["front"], o["graph"], LU.K, case.iv))
        return made[name]
    return get


def same_as_reference(name, cov, out):
    want, got = TABLE["window:" + name]["expected"][str(cov)], R.digest(out)
    assert got == want, "%s at coverage %d: the device differs from the reference in %s" % (name, cov, [k for k in R.KEYS if got[k] != want[k]])


def run_engine(agx, case, tmp, rebuild=False, reprune=()):
    got = {}
    with agx.Unit(k=LU.K, insert_variation=case.iv, coverage=case.coverage, keep_counts=True, edge_support=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        got["graph"] = u.graph()
        got["out"] = u.finish()
        got["stats"] = u.stats()
        got["support"] = u.edge_support()
        if rebuild:
            u.build()
            got["graph2"] = u.graph()
            got["out2"] = u.finish()
            got["support2"] = u.edge_support()
        got["repruned"] = {}
        for c in reprune:
            u.reprune(c)
            got["repruned"][c] = (u.finish(), u.edge_support())
    return got


def check(name, case, o, model, got, passes=True):
    assert WU.graph_diff(name, o["graph"], got["graph"]) is None, WU.graph_diff(name, o["graph"], got["graph"])
    same_as_reference(name, case.coverage, got["out"])
    # the passes that took the unit's tiles: what the oracle's variants per tile say (the cases assert on them which pass their edges sit in)
    st = got["stats"]
    assert not passes or (st["n_mid_tiles"], st["n_big_tiles"]) == (WU.tiles_beyond(o, 2), WU.tiles_beyond(o, 4)), (name, st["n_mid_tiles"], st["n_big_tiles"])
    assert st["n_nodes"] == int(o["graph"]["n_nodes"])
    assert model["off_graph"] == 0
    check_counts(got["support"], got["graph"], model)


@pytest.fixture(scope="module")
def engine_of(agx, unit_of):
    made = {}

    def get(name):
        if name not in made:
            case, tmp, o, model = unit_of(name)
            made[name] = run_engine(agx, case, tmp, rebuild=True, reprune=case.reprune)
        return made[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle_and_reference(engine_of, unit_of, name):
    case, tmp, o, model = unit_of(name)
    check(name, case, o, model, engine_of(name))


@pytest.mark.parametrize("name", list(CASES))
def test_second_build_of_the_resident_unit(engine_of, unit_of, name):
    case, tmp, o, model = unit_of(name)
    got = engine_of(name)
    assert WU.graph_diff(name, o["graph"], got["graph2"]) is None, WU.graph_diff(name, o["graph"], got["graph2"])
    same_as_reference(name, case.coverage, got["out2"])
    check_counts(got["support2"], got["graph2"], model)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.reprune])
def test_reprune_to_the_cases_coverages(engine_of, unit_of, name):
    case, tmp, o, model = unit_of(name)
    got = engine_of(name)
    assert sorted(got["repruned"]) == sorted(case.reprune)
    for cov, (out, support) in got["repruned"].items():
        same_as_reference(name, cov, out)
        check_counts(support, got["graph"], model)      # the counts do not depend on the prune


@pytest.mark.parametrize("env", ["AGX_UPLOAD_WINDOWS=3", "AGX_TEST_SMALL_CAPS=1"])
@pytest.mark.parametrize("name", list(CASES))
def test_case_under(agx, unit_of, name, env, monkeypatch):
    case, tmp, o, model = unit_of(name)
    monkeypatch.setenv(*env.split("="))
    check(name, case, o, model, run_engine(agx, case, tmp), passes="WINDOWS" in env)      # (with every capacity small a build is repeated: its pass counters are not compared)
