"""The cases of tests/sweep_units.py (passes 1, 2 and 3 of the node sweep, the lists between them, the node pool's slices and spill area) on the CPU: every unit
through the serial executor against the oracle, and every case's arms asserted from the oracle's graph and the model of sweep_units.py.  The executor sweeps a
tile with one bucket and takes ids from one counter, so it proves no more than that the inputs are valid, that the reference side stays inside every limit and
that each case reaches what it is there for; the device runs the same cases in tests/test_gpu_sweep_passes.py, on the same units (tests/sweep_fixture.py)."""
import numpy as np
import pytest

import forms_shim
import lean_units as LU
import sweep_units as SU
from conftest import graph_mismatch
from hostsim import sim
from sweep_fixture import CASES, swept  # noqa: F401  (swept: the fixture)

E_OVERFLOW = -7      # AGX_E_OVERFLOW (include/agx.h)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.overflow])
def test_case_matches_oracle_and_reaches_its_arms(swept, name):
    case, tmp, o, s, ctx = swept(name)
    assert graph_mismatch(o["graph"], s["graph"]) is None
    for key in ("initial", "pre", "extended"):
        assert o[key] == s[key], key
    SU.check_arms(case, ctx)
    assert s["n_big_tiles"] == ctx.n("mid")      # the executor's pass 0 gives up on a tile exactly where the model says the device's does
    assert ctx.n("huge") <= ctx.n("big") <= ctx.n("mid")


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.overflow])
def test_case_beyond_the_last_bucket_is_refused(swept, name):
    case, tmp, o, s, ctx = swept(name)
    SU.check_arms(case, ctx)      # the reference side: the oracle's own count
    with pytest.raises(sim.SimError) as e:
        sim.run(tmp, 0, LU.K, case.iv, case.coverage)
    assert e.value.code == E_OVERFLOW and str(SU.MAXV_HUGE) in e.value.msg


def test_stride_cases_outnumber_their_wavefronts(swept):
    """The counts the GPU file compares the device's statistics with, from the model: each list is longer than its pass has wavefronts."""
    got = {n: (swept(n)[4].n("mid"), swept(n)[4].n("big"), swept(n)[4].n("huge")) for n in ("stride_mid", "stride_big", "stride_huge")}
    print("mid, big, huge tiles:", got)
    assert got["stride_mid"][0] > SU.MID_WAVES and got["stride_mid"][1] > 0
    assert got["stride_big"][1] > 2 * SU.BIG_WAVES and got["stride_big"][2] == 0
    assert got["stride_huge"][2] > 2 * SU.HUGE_WAVES


def test_every_limit_has_a_case_at_its_value_and_one_beyond(swept):
    deepest = {n: int(swept(n)[4].per.max()) for n, c in CASES.items() if c.group == "limit"}
    for v in (SU.MAXV_LDS, SU.MAXV_MID, SU.MAXV_BIG, SU.MAXV_HUGE):
        assert v in deepest.values() and v + 1 in deepest.values(), v


def test_pool_plan_is_the_engines_first_layout(swept):
    """pool_plan against the figures of a 65 536-position unit (32 regions of 86 016 / 32 ids, a spill area of 73 728), and the spill case's region against them."""
    case, tmp, o, s, ctx = swept("spill")
    assert (ctx.share, ctx.spill, ctx.regions) == (2688, 73728, 32)
    d = int(ctx.demand[SU.SPILL_REGION])
    print("spill: region %d asks for %d ids, slice %d, spill area %d" % (SU.SPILL_REGION, d, ctx.share, ctx.spill))
    assert ctx.share < d <= ctx.spill
    assert int(ctx.demand.sum()) == int(o["graph"]["n_nodes"]) <= ctx.share * ctx.regions + ctx.spill
    # spilled ids are out of position order only if tiles behind the region still take ids from their slices
    assert int(np.nonzero(ctx.demand)[0].max()) > SU.SPILL_REGION


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.windows])
def test_window_cases_have_deep_tiles_in_two_windows(swept, name):
    """The cases the device sweeps again under AGX_UPLOAD_WINDOWS=3: pass 0 fills mid_list from more than one launch."""
    ctx = swept(name)[4]
    n_tiles = len(ctx.tmax)
    cuts = [n_tiles * w // 3 for w in range(4)]      # window w holds tiles n_tiles * w / W .. n_tiles * (w + 1) / W: the model, held to the engine's own cuts (agx_forms.h)
    assert forms_shim.window_cuts(n_tiles * 64, n_tiles, 3) == (3, cuts)
    assert sum(bool(((ctx.m["mid"] >= lo) & (ctx.m["mid"] < hi)).any()) for lo, hi in zip(cuts, cuts[1:])) >= 2
