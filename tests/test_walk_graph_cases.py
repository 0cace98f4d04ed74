"""The walk preparation on the CPU: the walk graph the serial executor hands to the host walk (hostsim.sim.run(..., walk=True)) against the independent model
of tests/walk_model.py, which works it out from the oracle's graph.  The cases of tests/walk_units.py first assert that their units reach the paths
they are there for; the hand-made units of the edge build and of pass 0, the golden vectors and two generated units go through the same comparison.
This proves the model without a device and pins the shared lane functions (agx_assign_aid_pos, agx_emit_alive_pos, agx_special_id, agx_walk_record)
against the oracle a second way; the device's own code for this stage runs the same cases in tests/test_gpu_walk_graph.py."""
import os

import pytest

import edge_units as EU
import harness as H
import lean_units as LU
import walk_model as WM
import walk_units as WU
from hostsim import sim

CASES = {c.name: c for c in WU.cases()}
OTHER = {"edge:" + c.name: c for c in EU.cases()}
OTHER.update({"lean:" + c.name: c for c in LU.cases()})


@pytest.fixture(scope="module")
def unit_of(built, tmp_path_factory):
    """Writes a case's unit and runs the oracle and the executor on it once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = WU.write_unit(case.unit, str(tmp_path_factory.mktemp(name)))
            made[name] = (case, tmp, H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True),
                          sim.run(tmp, 0, LU.K, case.iv, case.coverage, graph=True, walk=True))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_paths_and_matches_the_model(unit_of, name):
    case, tmp, o, s = unit_of(name)
    v = WU.check_paths(case, s)
    m = WM.build(o["graph"], case.coverage)
    assert WM.mismatch(m, s["walk"]) is None
    if case.special_ids:
        for a in case.special_ids(v):
            assert m["special"][a] and v.special[a], "%s: id %d is not special" % (name, a)
    for key in ("initial", "pre", "extended"):
        assert o[key] == s[key], key


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.sparse_min])
def test_case_with_side_ids_only_in_the_sparse_table(unit_of, name, monkeypatch):
    case, tmp, o, _ = unit_of(name)
    monkeypatch.setenv("AGX_SIM_SPARSE_MIN", "1")
    s = sim.run(tmp, 0, LU.K, case.iv, case.coverage, walk=True)
    m = WM.build(o["graph"], case.coverage, sparse_min=True)
    assert m["n_special"] == m["n_ids"] - m["n_pos"] > 0
    assert WM.mismatch(m, s["walk"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == s[key], key


def test_cases_reach_every_group_of_paths(unit_of):
    """Every group of paths has its cases, every case asserts at least one path of its own, and together they hold what no single case does."""
    assert {c.group for c in CASES.values()} == set(WU.GROUPS)
    assert all(c.want for c in CASES.values())
    views = {n: WU.View(unit_of(n)[3], CASES[n].coverage) for n in CASES}
    assert {255, 256, 257, 1023, 1024, 1025} <= {v.n_pos for v in views.values()} and any(v.n_pos > 4096 and v.n_pos % 1024 for v in views.values())
    assert any(len(v.ovf) > v.n_pos for v in views.values())                                     # overflow entries beyond the positions' grid
    assert any(v.n_seg0 == 0 for v in views.values()) and any(v.n_seg0 > 32 for v in views.values())
    assert any(v.n_words % 4 == 0 for v in views.values()) and any(v.n_words % 4 for v in views.values())
    kinds = set()
    for v in views.values():
        kinds |= set(v.kind.tolist())
    assert kinds == {"E", "A1", "P1", "VA", "VPA", "VPP"}


@pytest.mark.parametrize("name", list(OTHER))
def test_units_of_the_other_stages_match_the_model(built, tmp_path, name):
    case = OTHER[name]
    iv, cov = getattr(case, "iv", LU.IV), getattr(case, "coverage", 1)
    tmp = LU.write_unit(case.unit, str(tmp_path))
    o = H.run_oracle(tmp, 0, LU.K, iv, cov, graph=True)
    s = sim.run(tmp, 0, LU.K, iv, cov, walk=True)
    assert WM.mismatch(WM.build(o["graph"], cov), s["walk"]) is None


def test_golden_units_match_the_model(golden, built):
    p = golden.params
    for cov in p["coverages"]:
        for u in range(p["units"]):
            o = H.run_oracle(golden.tmp, u, p["k"], p["insert_variation"], cov, graph=True)
            s = sim.run(golden.tmp, u, p["k"], p["insert_variation"], cov, walk=True)
            assert WM.mismatch(WM.build(o["graph"], cov), s["walk"]) is None, "%s cov=%d unit=%d" % (golden.name, cov, u)


# two generated units with the settings of tests/test_gpu_parity.py: CONFIGS[0], and the unit of its sparse-table test (long contigs, the +1000 skip)
GENERATED = [dict(seed=201, chroms="60000", pairs=20000, coverage=5, contig_min=1500, contig_max=3000),
             dict(seed=105, chroms="300000", pairs=60000, coverage=5, contig_min=120000, contig_max=200000)]


@pytest.mark.parametrize("cfg", GENERATED, ids=lambda c: "seed%d" % c["seed"])
def test_generated_units_match_the_model(built, tmp_path, cfg):
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **cfg)
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    o = H.run_oracle(tmp, 0, meta["k"], meta["insert_variation"], meta["coverage"], graph=True)
    s = sim.run(tmp, 0, meta["k"], meta["insert_variation"], meta["coverage"], walk=True)
    m = WM.build(o["graph"], meta["coverage"])
    assert WM.mismatch(m, s["walk"]) is None
    assert m["n_special"] * 4 < m["n_ids"]
