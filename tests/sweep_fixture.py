"""What tests/test_sweep_cases.py and tests/test_gpu_sweep_passes.py share: the cases of tests/sweep_units.py, each written, run through the oracle and through the
serial executor ONCE per process (both files in one run use the same units and the same reference results, which nothing changes)."""
import pytest

import harness as H
import lean_units as LU
import sweep_units as SU
from hostsim import sim

CASES = {c.name: c for c in SU.cases()}
_made = {}


@pytest.fixture(scope="module")
def swept(built, tmp_path_factory):
    """name -> (case, tmp, the oracle's run with its graph, the executor's run or None where the unit must be refused, Ctx)"""
    def get(name):
        if name not in _made:
            case = CASES[name]
            tmp = case.write(str(tmp_path_factory.mktemp(name)))
            o = H.run_oracle(tmp, 0, LU.K, case.iv, case.coverage, graph=True)
            s = None
            if not case.overflow:
                s = sim.run(tmp, 0, LU.K, case.iv, case.coverage, graph=True, records=True)
                del s["records"]
            _made[name] = (case, tmp, o, s, SU.Ctx(o["graph"], None if s is None else s["tile_len"]))
        return _made[name]
    return get
