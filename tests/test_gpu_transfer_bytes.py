"""What a unit's stats say crossed PCIe (agx_engine.cpp: download_bytes, upload_bytes) against what can be known about it from outside.

(a) download_bytes, exactly, against arithmetic on the walk graph that Unit.walk_graph() hands out: a base and a meta byte per walk id, a bitmap word
    and a rank (8 + 4 bytes) per 64 ids and one more, a position per side id, a record and a hop entry (32 + 12 bytes) per special id, 8 bytes per
    overflow edge — in the one-piece and in the streamed form, on a unit too small to stream, on a unit with overflow edges and after finish() of a
    one-shot unit (whose graph cannot be dumped: its counts come from the stats).
(b) upload_bytes is the sum of the copies the upload queued: how the read rows are cut into windows does not change it, nor where the download will
    land; the rows as differences from the reference are fewer bytes; and nothing is sent that the unit's block of HBM does not hold.  The rows as
    differences are left out of the window comparison: each window's count bytes are clamped to whole 64-row blocks, so that total may move with the cuts."""
import os

import pytest

import edge_units as EU
import harness as H
import lean_units as LU
import walk_units as WU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def graph_bytes(n_pos, n_ids, n_special, n_ovf):
    return 2 * n_ids + (n_ids // 64 + 1) * 12 + (n_ids - n_pos) * 4 + n_special * (32 + 12) + n_ovf * 8


CASES = {"kinds": WU.case_kinds(), "layout_1025": WU.case_layout(1025), "edge:overflow": EU.case_overflow()}


@pytest.fixture(scope="module")
def unit_of(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            made[name] = (WU.write_unit(case.unit, str(tmp_path_factory.mktemp(name.replace(":", "_")))), getattr(case, "iv", LU.IV), getattr(case, "coverage", 1))
        return made[name]
    return get


@pytest.mark.parametrize("name,form", [("kinds", "whole"), ("kinds", "streamed"), ("layout_1025", "whole"), ("edge:overflow", "whole")])
def test_download_bytes_are_the_walk_graph(agx, unit_of, name, form, monkeypatch):
    tmp, iv, cov = unit_of(name)
    monkeypatch.setenv("AGX_STREAM_PIECES", "16")
    with agx.Unit(k=LU.K, insert_variation=iv, coverage=cov) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        w = u.walk_graph(streamed=(form == "streamed"))
        st = u.stats()
    n_ovf = len(w["ovf"])
    print(name, form, "n_pos", w["n_pos"], "n_ids", w["n_ids"], "n_special", w["n_special"], "n_ovf", n_ovf, "download_bytes", st["download_bytes"])
    if name == "layout_1025":
        assert w["n_pos"] < 4096
    if name == "edge:overflow":
        assert n_ovf > 0
    assert len(w["sp_node"]) == w["n_special"] and len(w["meta"]) == w["n_ids"]
    assert st["download_bytes"] == graph_bytes(w["n_pos"], w["n_ids"], w["n_special"], n_ovf)


def test_download_bytes_of_a_one_shot_unit(agx, unit_of):
    tmp, iv, cov = unit_of("kinds")
    with agx.Unit(k=LU.K, insert_variation=iv, coverage=cov, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        u.finish()
        st = u.stats()
    print("one-shot", st["n_walk_ids"], st["n_special"], st["n_edge_overflow"], st["download_bytes"])
    assert st["n_walk_ids"] >= CASES["kinds"].unit.genome_len and st["n_special"] > 0
    assert st["download_bytes"] == graph_bytes(CASES["kinds"].unit.genome_len, st["n_walk_ids"], st["n_special"], st["n_edge_overflow"])


def test_upload_bytes_are_the_copies(agx, built, tmp_path, monkeypatch):
    """The unit of test_gpu_parity.py's test_tile_ordered_upload_and_a_sweep_by_windows, cut down: rows that are no multiple of 16 bytes, listed bases, second hits."""
    run = H.synth(str(tmp_path / "run"), seed=83, chroms="40000", pairs=8000, L=57, coverage=4, read_indel=0.2, multi=0.3, multi_near=0.5, read_n=0.01, contig_overlap=0.3, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    want = H.run_oracle(tmp, 0, 5, 50, 4)
    monkeypatch.setenv("AGX_NO_CACHE", "1")

    def run_one(windows, flags=0, row_diff=False):
        monkeypatch.setenv("AGX_UPLOAD_WINDOWS", windows)
        if row_diff:
            monkeypatch.setenv("AGX_ROW_DIFF", "1")
        with agx.Unit(k=5, insert_variation=50, coverage=4, flags=flags) as u:
            u.load_files(tmp, 0)
            u.upload()
            u.build()
            out = u.finish()
            st = u.stats()
        monkeypatch.delenv("AGX_ROW_DIFF", raising=False)
        for key in ("initial", "pre", "extended"):
            assert out[key] == want[key], (windows, flags, row_diff, key)
        print("windows", windows, "flags", flags, "row_diff", row_diff, "upload_bytes", st["upload_bytes"], "device_bytes", st["device_bytes"], "rows_by_reference", st["rows_by_reference"])
        assert 0 < st["upload_bytes"] <= st["device_bytes"], (windows, flags, row_diff)
        assert (st["rows_by_reference"] > 0) == row_diff
        return st["upload_bytes"]

    plain = run_one("1")
    assert run_one("3") == plain and run_one("8") == plain
    assert run_one("3", flags=agx.AGX_FLAG_ONE_SHOT) == plain
    assert run_one("1", row_diff=True) < plain
