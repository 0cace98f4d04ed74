"""The units of tests/unitig_units.py on the CPU: every case reaches its arms (predicates on the piece model of its named windows and on the executor's overflow
dump), the piece model agrees with the export's model on what both state, and the two numpy models of the export (tests/unitig_model.py,
tests/unitig_region_model.py) and the id map of tests/path_model.py equal the plain reference of tests/unitig_plain.py field by field on every named window: these
units have shapes the models were never run on.  The device's own code runs the same cases in tests/test_gpu_unitig_cases.py."""
import numpy as np
import pytest

import harness as H
import lean_units as LU
import path_model as PM
import unitig_model as M
import unitig_plain as PL
import unitig_region_model as R
import unitig_units as UU
import walk_model as WM
import walk_units as WU
from hostsim import sim

CASES = {c.name: c for c in UU.cases()}


@pytest.fixture(scope="module")
def made(built, tmp_path_factory):
    """name -> (case, tmp, Ctx): the unit written, the oracle (and for the cases that read the overflow dump the executor) run once per module"""
    out = {}

    def get(name):
        if name not in out:
            case = CASES[name]
            tmp = WU.write_unit(case.unit, str(tmp_path_factory.mktemp(name)))
            g = H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True)["graph"]
            s = sim.run(tmp, 0, LU.K, case.iv, case.coverage, edges=True) if case.edges else None
            out[name] = (case, tmp, UU.Ctx(case, g, s))
        return out[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_arms(made, name):
    case, tmp, ctx = made(name)
    assert ctx.ref == M.read_reference(tmp, 0)[:ctx.n_pos]
    UU.check_arms(case, ctx)


@pytest.mark.parametrize("name", list(CASES))
def test_piece_model_agrees_with_the_export_model(made, name):
    """Heads, segment lengths and links as the piece model has them are the region model's."""
    case, tmp, ctx = made(name)
    for w in case.windows:
        P, t = ctx.pm(w), R.region_unitigs(ctx.g, w[0], w[1], w[2], ctx.ref)
        assert P.pos[P.heads].tolist() == t["head_pos"].tolist() and P.var[P.heads].tolist() == t["head_var"].tolist(), w
        assert [UU.seg_len(P, g) for g in range(len(P.chains))] == t["n_nodes"].tolist(), w
        assert sorted((int(P.seg_of[a]), int(P.seg_of[b])) for a, b in P.links) == list(zip(t["link_from"].tolist(), t["link_to"].tolist())), w
        assert sorted(P.pos[P.tails].tolist()) == sorted(t["last_pos"].tolist()), w


@pytest.mark.parametrize("name", list(CASES))
def test_models_equal_the_plain_reference(made, name):
    case, tmp, ctx = made(name)
    g, n = ctx.g, ctx.n_pos
    for lo, hi, cov in case.windows:
        want = PL.unitigs(g, lo, hi, cov, ctx.ref)[0]
        x = UU.table_mismatch(R.region_unitigs(g, lo, hi, cov, ctx.ref), want)
        assert x is None, "%s: region model, window [%d, %d) at %d: %s" % (name, lo, hi, cov, x and x[2])
    texts = set()
    for cov in (case.coverage,) + case.reprune:
        t = M.unitigs(g, cov, ctx.ref)
        x = UU.table_mismatch(t, PL.unitigs(g, 0, n, cov, ctx.ref)[0])
        assert x is None, "%s: whole model at %d: %s" % (name, cov, x and x[2])
        texts.add(M.gfa_text(t, 0))
    assert len(texts) == 1 + len(case.reprune), "%s: two of the whole export's thresholds ask the same question" % name
    if case.maps:
        wm = WM.build(g, case.coverage)
        for lo, hi, cov in case.maps:
            got, want = PM.id_map(g, case.coverage, lo, hi, cov, ctx.ref, wm)[0]["id_map"], PL.id_map(g, case.coverage, lo, hi, cov, ctx.ref)
            assert (got["n_pos"], got["n_ids"]) == (want["n_pos"], want["n_ids"])
            for f in UU.RUNS:
                assert got[f].tolist() == want[f], "%s: id map, window [%d, %d) at %d: %s" % (name, lo, hi, cov, f)
            assert len(want["id_first"]) > 0
            UU.check_map_shapes(case, (lo, hi, cov), want, wm["side_xpos"])


def test_the_cases_together():
    """Every case of the issue's table is there, and no test of the device's runs more than about 300 exports."""
    assert list(CASES) == ["straight", "strands_2", "strands_3", "branch_lanes", "fans", "islands", "bases", "map_edges"]
    assert all(len(c.windows) <= 140 for c in CASES.values())
