"""The edge build (agx_k_edge_sweep, agx_k_edge_jump, agx_k_edge_slow, agx_slot_insert; agx_kernels.hip) case by case: the units of tests/edge_units.py
through the HIP engine against the oracle — node and edge tables field by field, the three output files, the device's slow-list length
(agx_stats.n_edge_slow) against the serial executor's count in the device's rule, and the overflow list's appends.  Every case runs with pass J
beside pass B (the default) and with both on one stream (AGX_FLAG_TIME_SECTIONS); the cases with jumps across window cuts also with the upload cut
into 2 and 3 windows, the overflow cases also with every capacity starting small and through the unitig export.  tests/test_edge_build_cases.py
runs the same cases through the serial executor."""
import os

import numpy as np
import pytest

import edge_units as EU
import harness as H
import lean_units as LU
import unitig_model as M
from conftest import graph_mismatch
from hostsim import sim

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in EU.cases()}


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
    """Writes a case's unit, checks its paths on the serial executor and runs the oracle on it, once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = LU.write_unit(case.unit, str(tmp_path_factory.mktemp(name)))
            s = sim.run(tmp, 0, LU.K, case.iv, case.coverage, graph=True, edges=True)
            EU.check_edges(case, s)
            made[name] = (case, tmp, H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True), s)
        return made[name]
    return get


def run_engine(agx, case, tmp, flags=0, gfa=False):
    with agx.Unit(k=LU.K, insert_variation=case.iv, coverage=case.coverage, keep_counts=True, flags=flags) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        out = {"gfa": u.gfa(0)} if gfa else {}
        out.update(u.finish())
        out["stats"] = u.stats()
        out["graph"] = u.graph()
    return out


def check(o, s, g):
    assert graph_mismatch(o["graph"], g["graph"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == g[key], key
    st = g["stats"]
    assert st["n_edge_slow"] == len(s["slow"]), (st["n_edge_slow"], len(s["slow"]))
    # every overflow pair is listed at least once; J and B may list one twice, and which of a source's successors spill depends on the order of inserts
    deg = g["graph"]["edge_start"][1:].astype(np.int64) - g["graph"]["edge_start"][:-1].astype(np.int64)
    distinct = int((deg - 4).clip(min=0).sum())
    assert distinct == s["edges"]["ovf_distinct"]
    assert st["n_edge_overflow"] >= s["edges"]["ovf_appends"] and st["n_edge_overflow"] >= distinct
    if s["edges"]["ovf_dup_appends"]:
        assert st["n_edge_overflow"] > distinct


MODES = {"side_j": 0, "one_stream": 4}      # 4: AGX_FLAG_TIME_SECTIONS


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(agx, unit_of, name, mode):
    case, tmp, o, s = unit_of(name)
    check(o, s, run_engine(agx, case, tmp, flags=MODES[mode]))


@pytest.mark.parametrize("windows", ["2", "3"])
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.windows])
def test_case_swept_by_windows(agx, unit_of, name, windows, monkeypatch):
    case, tmp, o, s = unit_of(name)
    monkeypatch.setenv("AGX_UPLOAD_WINDOWS", windows)
    check(o, s, run_engine(agx, case, tmp))


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.overflow])
def test_overflow_case_small_caps_and_unitigs(agx, unit_of, name, monkeypatch):
    case, tmp, o, s = unit_of(name)
    want = M.unit_gfa(o["graph"], case.coverage, M.read_reference(tmp, 0), 0)
    g = run_engine(agx, case, tmp, gfa=True)
    assert g["gfa"] == want
    monkeypatch.setenv("AGX_TEST_SMALL_CAPS", "1")
    g = run_engine(agx, case, tmp, gfa=True)
    check(o, s, g)
    # the overflow list outgrew its first guess (4 entries under AGX_TEST_SMALL_CAPS) and the build was repeated with the list the counter asked for
    assert s["edges"]["ovf_appends"] > 4 and g["stats"]["n_edge_overflow"] > 4 and g["stats"]["build_attempts"] > 1
    assert g["gfa"] == want
