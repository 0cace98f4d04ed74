"""Every hand-made unit of the suite — lean_units, edge_units, walk_units, sweep_units, front_units, unitig_units and window_units — against what the REAL reference
wrote for it (tests/golden/hand_units_reference.json, made by tests/golden/make_hand_units_reference.py): the unit's input files still have the recorded md5s, and the
oracle AND the serial executor reproduce the reference's three output files at the case's coverage and at every coverage it names for a reprune.  Where oracle/_ref is
built the reference itself runs again on the same files.  This is what holds the oracle (the suite's judge everywhere else) to the reference on hand-made inputs, and
on the edges of the compatibility windows in particular."""
import pytest

import harness as H
from golden import make_hand_units_reference as R
from hostsim import sim

UNITS = {u.name: u for u in R.units()}
TABLE = R.load()


def test_the_table_names_every_unit_and_coverage():
    assert sorted(TABLE) == sorted(UNITS)
    for name, u in UNITS.items():
        assert sorted(TABLE[name]["expected"]) == sorted(str(c) for c in u.coverages), name
        assert TABLE[name]["insert_variation"] == u.iv, name


@pytest.mark.parametrize("name", list(UNITS))
def test_unit_matches_the_reference(built, tmp_path, name):
    u, rec = UNITS[name], TABLE[name]
    run = str(tmp_path / "run")
    tmp = u.write(run)
    assert R.inputs_md5(tmp) == rec["inputs_md5"], "the unit's files changed: regenerate tests/golden/hand_units_reference.json"
    for cov in u.coverages:
        want = rec["expected"][str(cov)]
        for who, run_it in (("oracle", H.run_oracle), ("executor", sim.run)):
            if who == "executor" and u.refused:
                with pytest.raises(sim.SimError, match="more than 1024 node variants"):
                    run_it(tmp, 0, R.K, u.iv, cov)
                continue
            got = R.digest(run_it(tmp, 0, R.K, u.iv, cov))
            assert got == want, "%s at coverage %d: the %s differs from the reference in %s" % (name, cov, who, [k for k in R.KEYS if got[k] != want[k]])
        if H.have_reference():
            live = R.run_reference(H, run, tmp, u.iv, cov)
            assert R.digest(live) == want, "%s at coverage %d: the reference no longer writes what the table records" % (name, cov)
