"""Unitig export on the MI355X (-m gpu): Unit.gfa() byte for byte against the numpy model on the oracle's graph (tests/unitig_model.py), the walk's outputs
unchanged by an export, the calls it refuses, and one full-size unit."""
import os
import time

import pytest

import harness as H
from conftest import write_pileup_unit
from test_gpu_parity import CONFIGS
import unitig_model as M

pytestmark = pytest.mark.gpu
HIGH = 1 << 30          # a coverage no read pile reaches: only contig nodes survive


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def engine_gfa(agx, tmp, unit, k, iv, cov, flags=0):
    with agx.Unit(k=k, insert_variation=iv, coverage=cov, keep_counts=True, flags=flags) as u:
        u.load_files(tmp, unit)
        u.upload()
        u.build()
        return u.gfa(unit), u.stats()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "seed%d" % c["seed"])
def test_gfa_matches_the_model_on_every_unit(agx, cfg, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **cfg)
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    for u in range(meta["units"]):
        ref = M.read_reference(tmp, u)
        for cov in (meta["coverage"], HIGH):
            o = H.run_oracle(tmp, u, meta["k"], meta["insert_variation"], cov, graph=True)
            want = M.unit_gfa(o["graph"], cov, ref, u)
            got, _ = engine_gfa(agx, tmp, u, meta["k"], meta["insert_variation"], cov)
            assert got == want, "seed %d unit %d coverage %d" % (cfg["seed"], u, cov)
            if cov == HIGH:
                assert all(line.startswith(b"S\t") or line.startswith(b"L\t") for line in got.splitlines())


def test_pileup_and_overflow_edges(agx, built, tmp_path):
    # a pile-up of 180 pairs on one left-mate alignment: 180 variants at each of its positions
    tmp = write_pileup_unit(str(tmp_path / "pile"), 180, spacing=300)
    o = H.run_oracle(tmp, 0, 5, 50, 1, graph=True)
    got, st = engine_gfa(agx, tmp, 0, 5, 50, 1)
    assert got == M.unit_gfa(o["graph"], 1, M.read_reference(tmp, 0), 0)
    assert got.count(b"S\t") >= 180
    # narrow windows on deep overlapping contigs: nodes with more than four successors, whose further edges sit on the overflow list (where an
    # edge can be listed twice)
    run = H.synth(str(tmp_path / "run"), seed=208, chroms="60000", pairs=20000, coverage=4, insert_variation=10, frag_sd=150, contig_overlap=0.4, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    for cov in (4, 1):
        o = H.run_oracle(tmp, 0, 5, 10, cov, graph=True)
        got, st = engine_gfa(agx, tmp, 0, 5, 10, cov)
        assert st["n_edge_overflow"] > 0
        assert got == M.unit_gfa(o["graph"], cov, M.read_reference(tmp, 0), 0)


def test_finish_after_an_export_is_unchanged(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), seed=211, chroms="60000", pairs=20000, coverage=5, contig_min=1500, contig_max=3000, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    outs = []
    for export in (False, True):
        with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True) as u:
            u.load_files(tmp, 0)
            u.upload()
            u.build()
            if export:
                assert u.unitigs()["seq"]
            outs.append(u.finish())
    assert outs[0] == outs[1]
    # one-shot units: before the download; the walk still gives the same bytes
    with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        u.unitigs()
        assert u.finish() == outs[0]
        with pytest.raises(agx.AgxError) as e:
            u.unitigs()
        assert e.value.code == agx.AGX_E_ARG


def test_refused_without_counts_and_after_trim(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), seed=212, chroms="30000", pairs=8000, coverage=5, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    with agx.Unit(k=5, insert_variation=50, coverage=5) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        with pytest.raises(agx.AgxError) as e:
            u.gfa(0)
        assert e.value.code == agx.AGX_E_ARG and "KEEP_COUNTS" in e.value.msg
    with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True) as u:
        u.load_files(tmp, 0)
        with pytest.raises(agx.AgxError) as e:
            u.unitigs()                 # not built
        assert e.value.code == agx.AGX_E_ARG
        u.upload()
        u.build()
        u.download()
        u.trim()
        with pytest.raises(agx.AgxError) as e:
            u.unitigs()
        assert e.value.code == agx.AGX_E_ARG


def test_full_size_unit_matches_the_model(agx, built, tmp_path):
    """cfg3's largest unit at full length (30.4 Mb, 3 M pairs of 2x100): export time against the graph dump + model on the same unit."""
    run = H.synth(str(tmp_path / "run"), seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
    tmp = os.path.join(run, "tmp")
    o = H.run_oracle(tmp, 0, 5, 50, 5, graph=True)
    t0 = time.time()
    want = M.unit_gfa(o["graph"], 5, M.read_reference(tmp, 0), 0)
    t_model = time.time() - t0
    with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        u.unitigs()                     # (first call: the kernels' code objects load)
        lib = agx.lib()
        import ctypes
        ms = []
        for _ in range(3):
            t = agx.Unitigs()
            t0 = time.perf_counter()
            rc = lib.agx_unit_unitigs(u._h, ctypes.byref(t))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == agx.AGX_OK
            p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
            t0 = time.perf_counter()
            assert lib.agx_unitigs_gfa(ctypes.byref(t), 0, ctypes.byref(p), ctypes.byref(n)) == agx.AGX_OK
            ms_gfa = (time.perf_counter() - t0) * 1e3
            got = ctypes.string_at(p, n.value)
            lib.agx_text_free(p)
            lib.agx_unitigs_free(ctypes.byref(t))
        t0 = time.time()
        u.graph()
        t_graph = time.time() - t0
    assert got == want
    print("full-size unitigs: %d nodes, %d S lines, %d bytes; agx_unit_unitigs %s ms, agx_unitigs_gfa %.1f ms; agx_unit_graph %.0f ms + model %.0f ms"
          % (o["graph"]["n_nodes"], got.count(b"S\t"), len(got), "/".join("%.1f" % x for x in ms), ms_gfa, t_graph * 1e3, t_model * 1e3))


def test_export_scratch_is_reserved_with_the_unit(agx, built, tmp_path):
    """A unit that keeps counts has the export's scratch in the block its upload takes (agx_unit_hbm_needed counts it, AlignGraph_amd admits units by
    it): the export asks the device for no further memory, however often it runs."""
    run = H.synth(str(tmp_path / "run"), seed=213, chroms="200000", pairs=40000, coverage=5, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    need = {}
    for keep in (False, True):
        with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=keep) as u:
            u.load_files(tmp, 0)
            need[keep] = u.hbm_needed()
    with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        before = u.stats()["device_bytes"]
        first = u.gfa(0)
        assert u.gfa(0) == first
        assert u.stats()["device_bytes"] == before
        n_pos = u.stats()["n_pos"]
    assert need[True] - need[False] >= 60 * n_pos          # (the counts, 24 bytes per node slot, and the export's scratch)
