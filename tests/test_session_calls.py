"""The table of the on-request calls (tests/session_calls.py) on the CPU: every kind has a model's answer to every one of its questions on every unit named for
tests/test_gpu_session.py, the questions reach what they are asked for (intervals under the thresholds, a middle window that is not the whole unit, overflow edges on the
executor's records, forks), and a comparator's text names the field and the index."""
import numpy as np
import pytest

import session_calls as SC

UNITS = SC.units()


@pytest.fixture(scope="module")
def modelled(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            u = UNITS[name]
            made[name] = SC.make_model(u, u.write(str(tmp_path_factory.mktemp(name))))
        return made[name]
    return get


@pytest.mark.parametrize("name", list(UNITS))
def test_every_kind_has_a_model_on_every_unit(modelled, name):
    m = modelled(name)
    kinds = SC.table(m)
    assert tuple(kinds) == SC.KINDS and len(SC.KINDS) == 11
    lo, hi = m["windows"]["middle"]
    assert 0 < lo < hi < m["n_pos"] and lo % 64 and hi % 64
    for k in SC.KINDS:
        want = kinds[k].want()
        assert len(want) == len(kinds[k].asks) >= (2 if k in SC.WINDOW_KINDS + SC.TABLE_KINDS else 1), k
        assert kinds[k].want() is want, "made once"
    for k in ("evidence", "walk_span"):      # thresholds that produce intervals, on the unit's own stretches or on the hand table
        assert sum(len(w["iv_rec"]) for w in kinds[k].want()) > 0, k
    assert len(kinds["unitigs"].want()[0]["head_pos"]) > 0 and len(kinds["edge_reads"].want()[0]["hit"]) == m["sup"]["n_contributions"] > 0
    assert len(m["tables"]["own"]["rec_len"]) > 0 and len(m["tables"]["interleaved"]["rec_len"]) == 3
    plain = SC.table(m, support=False)
    assert plain["evidence"].want()[0]["n_steps"] == 0 and not plain["bubbles"].want()[0]["has_support"] and kinds["bubbles"].want()[0]["has_support"]


def test_the_units_reach_what_the_kinds_are_asked_for(modelled):
    """Every kind runs on every unit, so on two at least; one of them has overflow edges by the executor's own record of its appends; somewhere there are links between
    records, bubbles with rows, and side ids under a table."""
    ovf = {n: modelled(n)["n_ovf"] for n in UNITS}
    assert len(UNITS) >= 2 and ovf["edge_overflow"] > 0, ovf
    assert any(SC.table(modelled(n))["bubbles"].want()[0]["n_bubbles_all"] > 0 for n in UNITS)
    assert any(len(SC.table(modelled(n))["mate_links"].want()[1]["a"]) > 0 for n in UNITS)
    assert any(modelled(n)["n_ids"] > modelled(n)["n_pos"] for n in UNITS)
    assert any(len(SC.table(modelled(n))["support"].want()[0][1]) > 100 for n in UNITS)


def test_a_difference_is_named_by_field_and_index(modelled):
    kinds = SC.table(modelled("walk_kinds"))
    assert SC.where("x", np.array([1, 2, 3]), np.array([1, 5, 3])) == "x[1] = 2, expected 5"
    assert SC.where("x", np.array([1, 2]), np.array([1, 2, 3])) == "x has 2 entries, expected 3"
    assert SC.where("seq", b"ACGT", b"ACCT") == "seq[2] = 71, expected 67"
    assert SC.where("n", 3, 4) == "n = 3, expected 4"
    for k in ("pair_span", "walk_span", "evidence", "mate_links", "edge_reads", "region"):
        want = kinds[k].want()
        assert kinds[k].same(want, want) is None, k
    got = [dict(w) for w in kinds["pair_span"].want()]
    got[1]["span"] = got[1]["span"].copy()
    got[1]["span"][5] += 1
    assert kinds["pair_span"].same(got, kinds["pair_span"].want()).startswith("pair_span, middle: span[5] = ")
    got = [dict(w) for w in kinds["region"].want()]
    got[0]["coverage"] = np.array(got[0]["coverage"]).copy()
    got[0]["coverage"][0] += 1
    assert kinds["region"].same(got, kinds["region"].want()).startswith("region, whole: coverage[0] = ")
    assert kinds["region"].same(got[:1], kinds["region"].want()) == "region: 1 answers, expected 3"
