"""Region export on the MI355X (-m gpu): Unit.gfa(unit, region, min_coverage) byte for byte against the region model on the oracle's graph
(tests/unitig_region_model.py), for windows whose edges sit around the wavefront size, thresholds below and above the build's coverage, a pile of 180
variants cut in the middle, windows that cut overflow edges; the whole export and the walk's outputs unchanged by any order of exports; the calls it
refuses; and one window of a full-size unit, timed against the whole export."""
import ctypes
import os
import random
import time

import numpy as np
import pytest

import harness as H
from conftest import write_pileup_unit
from test_gpu_parity import CONFIGS
import unitig_model as M
import unitig_region_model as R

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


def built_unit(agx, tmp, unit, k, iv, cov, flags=0, keep_counts=True):
    u = agx.Unit(k=k, insert_variation=iv, coverage=cov, keep_counts=keep_counts, flags=flags)
    u.load_files(tmp, unit)
    u.upload()
    u.build()
    return u


def config(seed):
    return next(c for c in CONFIGS if c["seed"] == seed)


@pytest.mark.parametrize("seed", [201, 203])
def test_whole_window_at_the_units_coverage_is_the_existing_export(agx, built, seed, tmp_path):
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **config(seed))
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    for unit in range(meta["units"]):
        k, iv, cov = meta["k"], meta["insert_variation"], meta["coverage"]
        o = H.run_oracle(tmp, unit, k, iv, cov, graph=True)
        n_pos = o["graph"]["n_pos"]
        with built_unit(agx, tmp, unit, k, iv, cov) as u:
            assert u.stats()["n_pos"] == n_pos
            whole = u.gfa(unit)
            assert whole.count(b"S\t") > 0
            assert u.gfa(unit, region=(0, n_pos), min_coverage=cov) == whole
            assert u.gfa(unit, region=(0, n_pos)) == whole              # region alone: the unit's own coverage
            assert u.gfa(unit, min_coverage=cov) == whole               # min_coverage alone: every position
            assert whole == R.region_gfa(o["graph"], 0, n_pos, cov, M.read_reference(tmp, unit), unit)
            a, b = u.unitigs(), u.unitigs(region=(0, n_pos), min_coverage=cov)
            assert sorted(a) == sorted(b) and all(np.array_equal(a[f], b[f]) for f in a if f != "seq") and a["seq"] == b["seq"]


def test_window_edges_at_the_wavefront_size(agx, built, tmp_path):
    cfg = config(203)                                                   # one 30 kb unit
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **cfg)
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    k, iv, cov = meta["k"], meta["insert_variation"], meta["coverage"]
    g = H.run_oracle(tmp, 0, k, iv, cov, graph=True)["graph"]
    ref, n = M.read_reference(tmp, 0), g["n_pos"]
    edges = [0, 1, 63, 64, 65, 127, 128, 129, n - 65, n - 64, n - 1, n]
    assert edges == sorted(edges)
    pairs = [(lo, hi) for lo in edges for hi in edges if lo <= hi]
    assert len(pairs) == 78
    with built_unit(agx, tmp, 0, k, iv, cov) as u:                      # one build, many exports
        nonempty = 0
        for lo, hi in pairs:
            got = u.gfa(0, region=(lo, hi))
            assert got == R.region_gfa(g, lo, hi, cov, ref, 0), "window [%d, %d)" % (lo, hi)
            nonempty += bool(got)
            if lo == hi:
                assert got == b""
        assert nonempty >= 40                                           # (the model gives text for 50 of them: the rest lie in front of the first read or are empty)


def test_thresholds_below_and_above_the_builds_coverage(agx, built, tmp_path):
    """The node table keeps the edges of the nodes the build pruned, so thresholds below the build's coverage are served, not refused."""
    cfg = config(201)                                                   # 60 kb with contigs, built at coverage 5
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **cfg)
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    k, iv, c = meta["k"], meta["insert_variation"], meta["coverage"]
    g = H.run_oracle(tmp, 0, k, iv, c, graph=True)["graph"]
    ref, n = M.read_reference(tmp, 0), g["n_pos"]
    rnd = random.Random(20)
    windows = []
    for _ in range(20):
        size = rnd.randint(1, 5000)
        lo = rnd.randint(0, n - size)
        windows.append((lo, lo + size))
    with built_unit(agx, tmp, 0, k, iv, c) as u:
        texts = {}
        for cov in (0, 1, c, c + 3, HIGH):
            for lo, hi in windows:
                got = u.gfa(0, region=(lo, hi), min_coverage=cov)
                assert got == R.region_gfa(g, lo, hi, cov, ref, 0), "window [%d, %d) at coverage %d" % (lo, hi, cov)
                texts[cov] = texts.get(cov, b"") + got
        # the thresholds are not all the same question on this unit
        assert len(set(texts.values())) >= 4
        assert texts[0].count(b"S\t") > texts[c].count(b"S\t") or texts[0].count(b"L\t") > texts[c].count(b"L\t")


def test_pileup_cut_in_the_middle_and_overflow_edges_cut_by_the_window(agx, built, tmp_path):
    # 180 variants at each position of one left-mate alignment (positions 1000 ..): a window that starts inside the pile has three wavefronts of local ids per position
    tmp = write_pileup_unit(str(tmp_path / "pile"), 180, spacing=300)
    g = H.run_oracle(tmp, 0, 5, 50, 1, graph=True)["graph"]
    ref = M.read_reference(tmp, 0)
    per_pos = np.diff(g["node_start"].astype(np.int64))
    assert per_pos[1050] == 180 and per_pos[1051] == 180
    with built_unit(agx, tmp, 0, 5, 50, 1) as u:
        for lo, hi in ((1050, 1051), (1050, 1053), (1040, 1200), (1050, 3000), (900, 1050)):
            got = u.gfa(0, region=(lo, hi), min_coverage=1)
            assert got == R.region_gfa(g, lo, hi, 1, ref, 0), "window [%d, %d)" % (lo, hi)
            if lo == 1050:
                assert got.count(b"S\t") >= 180
    # nodes with more than four successors: their further edges sit on the overflow list; windows that end between such a node's successors cut some of them
    run = H.synth(str(tmp_path / "run"), seed=208, chroms="60000", pairs=20000, coverage=4, insert_variation=10, frag_sd=150, contig_overlap=0.4, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    g = H.run_oracle(tmp, 0, 5, 10, 4, graph=True)["graph"]
    ref, n = M.read_reference(tmp, 0), g["n_pos"]
    node_start, es = g["node_start"].astype(np.int64), g["edge_start"].astype(np.int64)
    pos = np.repeat(np.arange(n, dtype=np.int64), np.diff(node_start))
    wide = np.nonzero(np.diff(es) > 4)[0]
    assert len(wide) > 0
    windows = [(0, n)]
    for s in wide[:: max(1, len(wide) // 6)][:6]:
        succ = np.sort(pos[g["edge_dst"][es[s]:es[s + 1]].astype(np.int64)])
        mid = int(succ[len(succ) // 2])
        windows.append((max(0, int(pos[s]) - 70), mid))                # the node inside, its later successors outside
        windows.append((int(pos[s]), int(succ[-1]) + 1))                # the node first in the window, every successor inside
        windows.append((int(pos[s]) + 1, min(n, int(succ[-1]) + 200)))  # the node itself outside
    with built_unit(agx, tmp, 0, 5, 10, 4) as u:
        assert u.stats()["n_edge_overflow"] > 0
        for cov in (4, 1):
            for lo, hi in windows:
                assert u.gfa(0, region=(lo, hi), min_coverage=cov) == R.region_gfa(g, lo, hi, cov, ref, 0), "window [%d, %d) at coverage %d" % (lo, hi, cov)


def test_exports_in_any_order_disturb_nothing(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), seed=211, chroms="60000", pairs=20000, coverage=5, contig_min=1500, contig_max=3000, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    g = H.run_oracle(tmp, 0, 5, 50, 5, graph=True)["graph"]
    ref, n = M.read_reference(tmp, 0), g["n_pos"]
    with built_unit(agx, tmp, 0, 5, 50, 5) as u:                        # never exports a region
        whole = u.gfa(0)
        fin = u.finish()
    windows = [(100, 5000, 1), (20000, n, 0), (0, n, HIGH), (5, 70, 5), (30000, 30001, 1), (0, n, 0)]
    want = {w: R.region_gfa(g, w[0], w[1], w[2], ref, 0) for w in windows}
    with built_unit(agx, tmp, 0, 5, 50, 5) as u:
        before = u.stats()["device_bytes"]
        for lo, hi, cov in windows[:3]:                                 # regions first, on scratch no export has touched
            assert u.gfa(0, region=(lo, hi), min_coverage=cov) == want[(lo, hi, cov)]
        assert u.gfa(0) == whole                                        # the whole export after regions
        for lo, hi, cov in reversed(windows):                           # regions after the whole export: its leftovers in the scratch and in the reverse map
            assert u.gfa(0, region=(lo, hi), min_coverage=cov) == want[(lo, hi, cov)]
        assert u.gfa(0) == whole
        assert u.gfa(0, region=(5, 70)) == want[(5, 70, 5)]
        assert u.stats()["device_bytes"] == before
        assert u.finish() == fin
    # one-shot units: before the download
    with built_unit(agx, tmp, 0, 5, 50, 5, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        assert u.gfa(0, region=(100, 5000), min_coverage=1) == want[(100, 5000, 1)]
        assert u.finish() == fin
        with pytest.raises(agx.AgxError) as e:
            u.gfa(0, region=(100, 5000), min_coverage=1)
        assert e.value.code == agx.AGX_E_ARG


def test_refusals(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), seed=212, chroms="30000", pairs=8000, coverage=5, sam_seq=0)
    tmp = os.path.join(run, "tmp")

    def refused(u, **kw):
        with pytest.raises(agx.AgxError) as e:
            u.gfa(0, **kw)
        assert e.value.code == agx.AGX_E_ARG
        return e.value.msg

    with built_unit(agx, tmp, 0, 5, 50, 5, keep_counts=False) as u:
        assert "KEEP_COUNTS" in refused(u, region=(0, 10))
    with agx.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True) as u:
        u.load_files(tmp, 0)
        refused(u, region=(0, 10))                                      # not built
        u.upload()
        u.build()
        n = u.stats()["n_pos"]
        msg = refused(u, region=(10, 9))
        assert "[10, 9)" in msg and str(n) in msg                      # the message names the bounds
        msg = refused(u, region=(0, n + 1))
        assert "[0, %d)" % (n + 1) in msg and "[0, %d)" % n in msg
        refused(u, region=(n + 1, n + 1))
        refused(u, region=(0, 1 << 32))                                 # (not a 32-bit number: refused by the binding)
        refused(u, region=(-1, 5))
        refused(u, min_coverage=-1)
        assert u.gfa(0, region=(n, n)) == b"" and u.gfa(0, region=(0, 0)) == b""
        t = u.unitigs(region=(7, 7))
        assert len(t["head_pos"]) == 0 and t["seq"] == b"" and t["seq_off"].tolist() == [0]
        assert u.gfa(0, region=(0, n))
        u.download()
        u.trim()
        refused(u, region=(0, 10))
        refused(u, min_coverage=1)


def test_a_window_of_a_full_size_unit(agx, built, tmp_path):
    """The 30.4 Mb unit of test_gpu_unitigs.test_full_size_unit_matches_the_model: a 100 000-position window in the middle against the model, and its wall time
    (minimum of three, after a warm-up call of each form) against the whole export's on the same unit in the same process.  Only the order is asserted."""
    run = H.synth(str(tmp_path / "run"), seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
    tmp = os.path.join(run, "tmp")
    g = H.run_oracle(tmp, 0, 5, 50, 5, graph=True)["graph"]
    n = g["n_pos"]
    lo = n // 2 - 50000
    hi = lo + 100000
    want = R.region_gfa(g, lo, hi, 5, M.read_reference(tmp, 0), 0)
    assert want.count(b"S\t") > 100
    lib = agx.lib()
    with built_unit(agx, tmp, 0, 5, 50, 5) as u:
        got = u.gfa(0, region=(lo, hi), min_coverage=5)                 # (first calls: the kernels' code objects load)
        u.unitigs()
        ms_region, ms_whole = [], []
        for _ in range(3):
            t = agx.Unitigs()
            t0 = time.perf_counter()
            rc = lib.agx_unit_unitigs_region(u._h, lo, hi, 5, ctypes.byref(t))
            ms_region.append((time.perf_counter() - t0) * 1e3)
            assert rc == agx.AGX_OK
            segs = t.n_segs
            lib.agx_unitigs_free(ctypes.byref(t))
            t = agx.Unitigs()
            t0 = time.perf_counter()
            rc = lib.agx_unit_unitigs(u._h, ctypes.byref(t))
            ms_whole.append((time.perf_counter() - t0) * 1e3)
            assert rc == agx.AGX_OK
            lib.agx_unitigs_free(ctypes.byref(t))
        again = u.gfa(0, region=(lo, hi), min_coverage=5)
        n_ovf = u.stats()["n_edge_overflow"]
    print("full-size unit, %d positions, %d overflow edges: window [%d, %d) gives %d segments, %d bytes of GFA; agx_unit_unitigs_region %s ms, agx_unit_unitigs %s ms"
          % (n, n_ovf, lo, hi, segs, len(got), "/".join("%.2f" % x for x in ms_region), "/".join("%.2f" % x for x in ms_whole)))
    assert got == want and again == want
    assert min(ms_region) < min(ms_whole)
