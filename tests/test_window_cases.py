"""The cases of tests/window_units.py (the compatibility windows at their edges: clause C, clause B and clause A, on the node side and the edge side) through the serial
executor against the oracle: node and edge tables with their counts, and the three output files.  Each case first asserts, on the oracle's graph and the executor's
records and counters, that its unit really sits on the edge it is there for and takes the path it names.  The device runs the same cases in
tests/test_gpu_window_cases.py; tests/test_hand_units_reference.py holds the oracle and the executor on these units against what the reference itself wrote."""
import pytest

import harness as H
import lean_units as LU
import window_units as WU
from conftest import graph_mismatch
from hostsim import sim

CASES = {c.name: c for c in WU.cases()}


@pytest.fixture(scope="module")
def unit_of(built, tmp_path_factory):
    """Writes a case's unit and runs the oracle and the executor on it once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = case.write(str(tmp_path_factory.mktemp(name)))
            made[name] = (case, tmp, H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True),
                          sim.run(tmp, 0, LU.K, case.iv, case.coverage, graph=True, edges=True, records=True))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_case_sits_on_its_edge(unit_of, name):
    case, tmp, o, s = unit_of(name)
    WU.check(case, o, s)


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(unit_of, name):
    case, tmp, o, s = unit_of(name)
    assert WU.graph_diff(name, o["graph"], s["graph"]) is None, WU.graph_diff(name, o["graph"], s["graph"])
    assert graph_mismatch(o["graph"], s["graph"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == s[key], key


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.reprune])
def test_case_matches_oracle_at_its_other_coverages(unit_of, name):
    case, tmp, o, s = unit_of(name)
    for cov in case.reprune:
        want, got = H.run_oracle(tmp, 0, LU.K, case.iv, cov), sim.run(tmp, 0, LU.K, case.iv, cov)
        for key in ("initial", "pre", "extended"):
            assert want[key] == got[key], (cov, key)
