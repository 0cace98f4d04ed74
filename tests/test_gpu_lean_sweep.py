"""Pass 0 of the node sweep (agx_sweep_tile_lean, agx_kernels.hip) case by case: the units of tests/lean_units.py — every lean record kind on both strands, the
lane edges, the 62-entry flush of the register counters, the limits of the packed counters, node variants and the slow path — through the HIP engine
against the oracle: node and edge tables field by field (vote counters included), the three output files, the sweep passes' statistics.  No CPU code runs
this loop; tests/test_lean_sweep_cases.py runs the same cases through the serial executor."""
import os

import pytest

import harness as H
import lean_units as LU
from conftest import graph_mismatch
from hostsim import sim

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in LU.cases()}


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
    """Writes a case's unit, checks its record shapes on the serial executor and runs the oracle on it, once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = LU.write_unit(case.unit, str(tmp_path_factory.mktemp(name)))
            LU.check_shapes(case, sim.run(tmp, 0, LU.K, LU.IV, 1, records=True))
            made[name] = (case, tmp, H.run_oracle(tmp, 0, LU.K, LU.IV, 1, graph=True))
        return made[name]
    return get


def run_engine(agx, tmp):
    with agx.Unit(k=LU.K, insert_variation=LU.IV, coverage=1, keep_counts=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        out = u.finish()
        out["stats"] = u.stats()
        out["graph"] = u.graph()
    return out


def check(case, o, g):
    assert graph_mismatch(o["graph"], g["graph"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == g[key], key
    for name, want in case.stats.items():
        assert want(g["stats"][name]) if callable(want) else g["stats"][name] == want, (name, g["stats"][name])


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(agx, unit_of, name):
    case, tmp, o = unit_of(name)
    check(case, o, run_engine(agx, tmp))


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.group in "ABCDE"])
def test_case_swept_by_windows(agx, unit_of, name, monkeypatch):
    # the same records met by the sweep window by window as the pieces of the upload land
    case, tmp, o = unit_of(name)
    monkeypatch.setenv("AGX_UPLOAD_WINDOWS", "3")
    check(case, o, run_engine(agx, tmp))
