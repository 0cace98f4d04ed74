"""The walk preparation on the device (agx_k_assign_aid, agx_k_emit_alive, agx_k_special_bits, the rank scan, agx_k_special_emit, agx_k_fetch_records;
agx_kernels.hip) and the download that carries its arrays to the host (do_download, begin_streamed_download; agx_engine.cpp): the walk graph as
Unit.walk_graph() copies it out, in both download forms, against the model of tests/walk_model.py (from the oracle's graph) and, in every field that
is defined bit for bit, against the serial executor's; the full record table through the fetch path against the model; finish() after the dump
against the oracle's three files.  Most of this stage's device code has no CPU twin (the kernels finish one-variant positions from registers, build
the special records level by level and take the hop entries from the runs), so the comparison has no tolerance: the only freedoms are the order
of a record's slots, which successors of a spilled node are in the slots, and NONE or repeated overflow entries.  tests/test_walk_graph_cases.py runs
the same cases on the CPU.

A streamed download needs window cuts: units below 4 096 positions have none (stream_cuts, agx_engine.cpp) and the hook must refuse that form with
AGX_E_ARG; every larger unit is cut by AGX_STREAM_PIECES.  Only the layout units of fixed small sizes and layout_min are below that; every case that runs in a
further mode (windows, pieces, small capacities, sparse-min) is large enough and must stream: those tests assert it.  The engine caps the pieces at n_pos / 1024, so
AGX_STREAM_PIECES=16 gives 16 windows on `kinds` (16 K positions), 10 on `hops`, 8 on `ovf_marks` and `no_contigs`, 4 on `last_side`."""
import os

import pytest

import edge_units as EU
import harness as H
import lean_units as LU
import walk_units as WU
from gpu_checks import check_walk as check
from hostsim import sim

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in WU.cases()}
OTHER = {"edge:" + c.name: c for c in EU.cases() if c.overflow or c.windows}
OTHER["lean:contimers"] = LU.case_contimers()
FORMS = ("whole", "streamed")


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
            case = CASES.get(name) or OTHER[name]
            iv, cov = getattr(case, "iv", LU.IV), getattr(case, "coverage", 1)
            tmp = WU.write_unit(case.unit, str(tmp_path_factory.mktemp(name.replace(":", "_"))))
            s = sim.run(tmp, 0, LU.K, iv, cov, graph=True, walk=True)
            if name in CASES:
                WU.check_paths(case, s)
            made[name] = (tmp, iv, cov, H.run_oracle(tmp, 0, LU.K, iv, cov, graph=True), s)
        return made[name]
    return get


def run_engine(agx, tmp, k, iv, cov, forms, flags=0, unit=0):
    """One unit: build, the walk graph in each of `forms` (with every record through the fetch path), then finish."""
    with agx.Unit(k=k, insert_variation=iv, coverage=cov, flags=flags) as u:
        u.load_files(tmp, unit)
        u.upload()
        u.build()
        dumps = [u.walk_graph(streamed=(f == "streamed"), all_node=True) for f in forms]
        out = u.finish()
        out["stats"] = u.stats()
    return dumps, out


def streams(o):
    return o["graph"]["n_pos"] >= 4096


def refused(agx, tmp, iv, cov):
    """A unit too small for window cuts: the streamed form is refused with a clear error, and the unit still finishes."""
    with agx.Unit(k=LU.K, insert_variation=iv, coverage=cov) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        with pytest.raises(agx.AgxError) as e:
            u.walk_graph(streamed=True)
        assert e.value.code == agx.AGX_E_ARG and "streamed" in e.value.msg
        return u.finish()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES) + list(OTHER))
def test_case_matches_the_model(agx, unit_of, name, form, monkeypatch):
    tmp, iv, cov, o, s = unit_of(name)
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    if form == "streamed" and not streams(o):
        out = refused(agx, tmp, iv, cov)
        for key in ("initial", "pre", "extended"):
            assert out[key] == o[key], key
        return
    dumps, out = run_engine(agx, tmp, LU.K, iv, cov, [form])
    check(o, dumps, out, cov, executor=s["walk"])


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.jumps])
def test_case_swept_by_windows_and_streamed_in_pieces(agx, unit_of, name, monkeypatch):
    tmp, iv, cov, o, s = unit_of(name)
    monkeypatch.setenv("AGX_UPLOAD_WINDOWS", "3")
    for pieces in ("2", "16"):
        monkeypatch.setenv("AGX_STREAM_PIECES", pieces)
        assert streams(o)
        dumps, out = run_engine(agx, tmp, LU.K, iv, cov, FORMS)
        check(o, dumps, out, cov, executor=s["walk"])


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.small_caps])
def test_case_with_every_capacity_too_small(agx, unit_of, name, monkeypatch):
    """AGX_TEST_SMALL_CAPS: the sparse table's first capacity is too small for the special records (agx_k_special_emit's `at >= sp_cap`), the build is repeated."""
    tmp, iv, cov, o, s = unit_of(name)
    monkeypatch.setenv("AGX_TEST_SMALL_CAPS", "1")
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    assert streams(o)
    dumps, out = run_engine(agx, tmp, LU.K, iv, cov, FORMS)
    check(o, dumps, out, cov, executor=s["walk"])
    assert out["stats"]["build_attempts"] > 1


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.sparse_min])
def test_case_with_side_ids_only_in_the_sparse_table(agx, unit_of, name, monkeypatch):
    """AGX_FLAG_SPARSE_MIN: only the side ids are special; every main record comes through agx_k_fetch_records and equals the model."""
    tmp, iv, cov, o, s = unit_of(name)
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    assert streams(o)
    dumps, out = run_engine(agx, tmp, LU.K, iv, cov, FORMS, flags=agx.AGX_FLAG_SPARSE_MIN)
    m = check(o, dumps, out, cov, sparse_min=True)
    assert m["n_special"] == m["n_ids"] - m["n_pos"] > 0


def test_golden_units_match_the_model(agx, golden, built, monkeypatch):
    p = golden.params
    monkeypatch.setenv("AGX_STREAM_PIECES", "3")
    streamed = 0
    for cov in p["coverages"]:
        for u in range(p["units"]):
            o = H.run_oracle(golden.tmp, u, p["k"], p["insert_variation"], cov, graph=True)
            dumps, out = run_engine(agx, golden.tmp, p["k"], p["insert_variation"], cov, FORMS if streams(o) else FORMS[:1], unit=u)      # (a fixture's units have the sizes they have)
            check(o, dumps, out, cov)
            streamed += streams(o)
    assert streamed, "no unit of %s is large enough to stream" % golden.name


def test_generated_unit_with_long_contigs_matches_the_model(agx, built, tmp_path, monkeypatch):
    """The unit of test_gpu_parity.py's sparse-table test (seed 105: long contigs, long records, the +1000 skip)."""
    run = H.synth(str(tmp_path / "run"), seed=105, chroms="300000", pairs=60000, coverage=5, contig_min=120000, contig_max=200000, sam_seq=0)
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    monkeypatch.setenv("AGX_STREAM_PIECES", "5")
    o = H.run_oracle(tmp, 0, meta["k"], meta["insert_variation"], meta["coverage"], graph=True)
    s = sim.run(tmp, 0, meta["k"], meta["insert_variation"], meta["coverage"], walk=True)
    dumps, out = run_engine(agx, tmp, meta["k"], meta["insert_variation"], meta["coverage"], FORMS)
    check(o, dumps, out, meta["coverage"], executor=s["walk"])


def test_one_shot_unit_refuses_the_dump(agx, unit_of):
    tmp, iv, cov, o, s = unit_of("special")
    with agx.Unit(k=LU.K, insert_variation=iv, coverage=cov, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        with pytest.raises(agx.AgxError) as e:
            u.walk_graph()
        assert e.value.code == agx.AGX_E_ARG and "one-shot" in e.value.msg
        out = u.finish()
    for key in ("initial", "pre", "extended"):
        assert out[key] == o[key], key
