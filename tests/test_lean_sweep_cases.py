"""The cases of tests/lean_units.py (every arm and limit of pass 0 of the node sweep) through the serial executor, on unpacked and on packed buckets
(agx_bucket::packed, the device's pass-0 layout: agx_cnt_word / agx_cnt_init / agx_cnt_get and the 16-bit halves), against the oracle.  Each case first
asserts that its units really make the lean record shapes it is there for.  The device runs the same cases in tests/test_gpu_lean_sweep.py."""
import pytest

import harness as H
import lean_units as LU
from conftest import graph_mismatch
from hostsim import sim

CASES = {c.name: c for c in LU.cases()}


@pytest.fixture(scope="module")
def unit_of(built, tmp_path_factory):
    """Writes a case's unit and runs the oracle on it once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = LU.write_unit(case.unit, str(tmp_path_factory.mktemp(name)))
            made[name] = (case, tmp, H.run_oracle(tmp, 0, LU.K, LU.IV, 1, graph=True))
        return made[name]
    return get


@pytest.mark.parametrize("packed", [False, True], ids=["unpacked", "packed"])
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(unit_of, name, packed):
    case, tmp, o = unit_of(name)
    s = sim.run(tmp, 0, LU.K, LU.IV, 1, graph=True, packed=packed, records=True)
    LU.check_shapes(case, s)
    assert graph_mismatch(o["graph"], s["graph"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == s[key], key
    # pass 0 of the executor gives up on a tile exactly where the device's pass 0 does (n_mid_tiles), but for the list of 65 536 entries only on packed buckets
    mid = case.stats.get("n_mid_tiles")
    if mid is not None and (packed or case.group != "F"):
        assert mid(s["n_big_tiles"]) if callable(mid) else s["n_big_tiles"] == mid


@pytest.mark.parametrize("n", [65535, 65536])
def test_packed_case_counters_reach_the_limit(unit_of, n):
    case, tmp, o = unit_of("packed_%d" % n)
    s = sim.run(tmp, 0, LU.K, LU.IV, 1, records=True)
    assert int(s["tile_len"].max()) == n
    cnt = o["graph"]["node_cnt"]
    assert (cnt[:, [0, 1, 3, 5]].max(axis=0) == n).all()      # coverage, and each high half of a packed counter word (A, G, N), at n somewhere


def test_vote_case_fills_all_five_fields(unit_of):
    case, tmp, o = unit_of("votes")
    cnt = o["graph"]["node_cnt"]
    assert int(((cnt[:, 1:] > 0).all(axis=1)).sum()) >= 2      # (one position per strand)
