"""CPU twin of tests/test_gpu_front.py: every hand-made unit of tests/front_units.py through the serial executor with its front dumped (hostsim.sim.run(..., front=True)).
The arm each case is there for is asserted from the model's predicates, the executor's tile lists, offsets and counts must be the plain model's (tests/front_model.py),
its copy of the unit sequence the file's bytes, its lean records must name the hits and rows its lists name, and its three outputs must be the oracle's."""
import numpy as np
import pytest

import front_model as FM
import front_units as FU
import harness as H
import lean_units as LU
from hostsim import sim

CASES = {c.name: c for c in FU.cases()}


@pytest.fixture(scope="module")
def run_of(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = FU.write_unit(case, str(tmp_path_factory.mktemp(name)))
            made[name] = (tmp, sim.run(tmp, 0, LU.K, LU.IV, 1, front=True, records=True))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_arm_and_the_executor_matches_the_model(run_of, name):
    case = CASES[name]
    tmp, s = run_of(name)
    f = s["front"]
    v = FU.View(case, f, tmp)
    FU.check_arms(case, v)
    m = v.m
    assert int(f["n_hits"]) == m["n_hits"] and int(f["n_tiles"]) == m["n_tiles"]
    assert np.array_equal(f["tile_off"].astype(np.int64), m["tile_off"]), "tile offsets"
    assert np.array_equal(np.diff(f["tile_off"].astype(np.int64)), m["tile_cnt"][:m["n_tiles"]]), "tile counts"
    assert np.array_equal(f["tile_recs"]["hit"].astype(np.int64), m["entry_hit"]), "the lists' hits"
    assert np.array_equal(f["tile_recs"]["slot"], f["dhit"]["a_slot"][m["entry_hit"]]), "the lean records' rows"
    # records=True's seven words are the same records without slot and hit
    r = s["records"]
    assert np.array_equal(r["tile"].astype(np.int64), m["entry_tile"])
    for word in ("geo", "qoff1", "boff1", "qoff2", "boff2", "lenjs"):
        assert np.array_equal(r[word], f["tile_recs"][word]), word
    assert f["ref"] == v.file_ref, "the unit sequence"
    assert len(f["cm_start"]) == v.n_pos + 1 and int(f["cm_start"][-1]) == int(f["n_cm"]) and np.array_equal(np.diff(f["cm_start"].astype(np.int64)), f["cm_head"]["n"][:v.n_pos])
    assert m["lookback"] == FM.lookback(case.L, LU.K)


@pytest.mark.parametrize("name", list(CASES))
def test_case_outputs_match_the_oracle(run_of, name):
    tmp, s = run_of(name)
    o = H.run_oracle(tmp, 0, LU.K, LU.IV, 1, graph=True)
    for key in ("initial", "pre", "extended"):
        assert s[key] == o[key], key
    # what the oracle itself holds per position: its base and its conti-mers
    f = s["front"]
    assert o["graph"]["pos_nuc"] == f["ref"]
    assert np.array_equal(o["graph"]["cm_count"], f["cm_head"]["n"][:int(f["n_pos"])])
