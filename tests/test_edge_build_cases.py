"""The cases of tests/edge_units.py (the paths of the edge build: pass A's boundary blocks and wave loop, the node sweep's slow listing, pass J,
pass B's register and general paths, the overflow list) through the serial executor against the oracle.  Each case first asserts that its unit
really reaches the paths it is there for.  The device runs the same cases in tests/test_gpu_edge_build.py."""
import pytest

import edge_units as EU
import harness as H
import lean_units as LU
from conftest import graph_mismatch
from hostsim import sim

CASES = {c.name: c for c in EU.cases()}


@pytest.fixture(scope="module")
def unit_of(built, tmp_path_factory):
    """Writes a case's unit and runs the oracle and the executor on it once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = LU.write_unit(case.unit, str(tmp_path_factory.mktemp(name)))
            made[name] = (case, tmp, H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True),
                          sim.run(tmp, 0, LU.K, case.iv, case.coverage, graph=True, edges=True))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(unit_of, name):
    case, tmp, o, s = unit_of(name)
    EU.check_edges(case, s)
    assert graph_mismatch(o["graph"], s["graph"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == s[key], key
    # the overflow list holds each source's edges beyond AGX_MAXE once per distinct pair
    deg = o["graph"]["edge_start"][1:].astype(int) - o["graph"]["edge_start"][:-1].astype(int)
    assert s["edges"]["ovf_distinct"] == int((deg - 4).clip(min=0).sum())
    assert len(s["slow"]) == s["edges"]["slow_sweep"] + s["edges"]["slow_a"]


def test_cases_reach_every_counter(unit_of):
    total = dict.fromkeys(sim.EDGE_COUNTERS, 0)
    for name in CASES:
        for k, v in unit_of(name)[3]["edges"].items():
            total[k] += v
    missing = sorted(k for k, v in total.items() if v == 0)
    assert not missing, missing
    assert total["ovf_dup_appends"] >= 1 and total["slow_tile_len_max"] > 64 and total["ovf_run_max"] >= 4

