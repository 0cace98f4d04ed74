"""The engine refuses damaged staged-pairs and cache files (tests/damaged_inputs.py, DESIGN.md "Rejected inputs"), on the device box.

Only entries of the table whose verdict is a REFUSAL take part — the CPU tests (tests/test_damaged_inputs.py) hold each to its rule — one or two per section and header,
taken by name.  What is asserted is that the refusal happens where the file is read, before anything is uploaded: load_files raises AGX_E_FORMAT with the rule's name for a
staged-pairs file; for a cache file stats()["from_cache"] == 0 is asserted BEFORE upload() is called, so a failing assertion ends the test with nothing sent to the device,
and the unit then built is the text's.  No test here uploads or builds from content the checks accepted in damaged form: what the checks let through is looked at on the
CPU, under the host sanitizers (tests/damaged_inputs_san.cpp), never here."""
import os

import pytest

import damaged_inputs as D
import harness as H
from test_damaged_inputs import K, SMALL

pytestmark = pytest.mark.gpu

PAIRS_ENTRIES = ["hit_row_n_rows", "hit_len_0", "hit1_back_2", "hit_side_runs2_n_sides", "hit_flag_bit_128_reverse", "side_runs2_end_n_runs_plus_1", "run_ends_past_read_end_forward",
                 "runs_of_a_mate_swapped", "other_mate_ends_past_unit_end_reverse", "jump_entry_nh", "jump_names_single_run_hit", "other_entries_swapped", "pairs_n_runs_plus_1", "pairs_stride_plus_1"]
CACHE_ENTRIES = ["hit_row_n_rows", "side_runs1_end_n_runs_plus_1", "run_ends_past_read_end_reverse", "other_mate_ends_past_unit_end_forward", "jump_entries_swapped", "other_entry_n_bases",
                 "seg_end_n_pos_plus_1", "cm_cnt_plus_1", "seg_rank_count", "chain_end_n_pos", "row_offset_past", "cache_nh_plus_1", "cache_len_rows_plus_1_row"]
COV = 4


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


@pytest.fixture(scope="module")
def small(built, tmp_path_factory):
    run = H.synth(str(tmp_path_factory.mktemp("gpu_damaged") / "run"), **SMALL)
    tmp = os.path.join(run, "tmp")
    return tmp, H.run_oracle(tmp, 0, K, 50, COV)


def build_and_compare(u, want):
    u.upload(); u.build()
    got = u.finish()
    for key in ("initial", "pre", "extended"):
        assert got[key] == want[key], key


def test_only_refused_entries_are_used():
    for name in PAIRS_ENTRIES + CACHE_ENTRIES:
        assert D.BY_NAME[name].verdict != D.ACCEPTED and D.BY_NAME[name].verdict in D.rule_names(), name
    assert all("pairs" in D.BY_NAME[n].doors for n in PAIRS_ENTRIES) and all({"cache", "cache_fast", "cache_header"} & set(D.BY_NAME[n].doors) for n in CACHE_ENTRIES)


def test_damaged_pairs_file_is_refused_at_load(agx, small, tmp_path):
    tmp, want = small
    path = os.path.join(tmp, "_agx_pairs.0.bin")
    cpu = D.CacheDoor(tmp, 0, K)
    n_pos = cpu.n["n_pos"]
    cpu.close()
    door = D.PairsDoor(path, n_pos, str(tmp_path), K, 1000000)
    with agx.Unit(k=K, insert_variation=50, coverage=COV) as u:
        try:
            for name in PAIRS_ENTRIES:
                e = D.BY_NAME[name]
                door.restore()
                e.apply(door)
                door.write(path)
                with pytest.raises(agx.AgxError) as err:
                    u.load_files(tmp, 0)
                assert err.value.code == agx.AGX_E_FORMAT and "(%s)" % e.verdict in err.value.msg, (name, err.value.code, err.value.msg)
        finally:
            with open(path, "wb") as f:
                f.write(door.bytes0)
        u.load_files(tmp, 0)                                   # the file as it was: the same Unit loads it, builds, and gives the oracle's outputs
        assert u.stats()["from_cache"] == 0 and u.stats()["n_hits"] == door.n["nh"]
        build_and_compare(u, want)


def test_damaged_cache_file_falls_back_to_the_text(agx, small, tmp_path):
    tmp, want = small
    pairs = os.path.join(tmp, "_agx_pairs.0.bin")
    keep = os.path.join(str(tmp_path), "_agx_pairs.0.bin")
    os.replace(pairs, keep)                                    # without the staged file the cache is made of the text (its rows are offsets into the reads file)
    try:
        agx.cache_build(tmp, 0, k=K)
        door = D.CacheFileDoor(os.path.join(tmp, "_agx_unit.0.bin"), reads_size=os.path.getsize(os.path.join(tmp, "_reads.fa")))
        used = 0
        for name in CACHE_ENTRIES:
            e = D.BY_NAME[name]
            if e.section == "rows" and door.kind not in e.doors:
                continue                                       # (an entry for the other kind of rows: read slots)
            used += 1
            door.restore()
            e.apply(door)
            door.write()
            with agx.Unit(k=K, insert_variation=50, coverage=COV) as u:
                u.load_files(tmp, 0)
                from_cache = u.stats()["from_cache"]
                assert from_cache == 0, "%s: the damaged cache file was taken" % name      # BEFORE upload: nothing of a damaged file may reach the device
                build_and_compare(u, want)
        assert used >= 11
        os.remove(door.path)
        agx.cache_build(tmp, 0, k=K)                           # a fresh cache is taken
        with agx.Unit(k=K, insert_variation=50, coverage=COV) as u:
            u.load_files(tmp, 0)
            assert u.stats()["from_cache"] == 1
            build_and_compare(u, want)
    finally:
        os.replace(keep, pairs)
