"""The compact wire forms of the hit and side records on the device (agx_k_expand_hits, agx_k_side_counts, agx_k_side_listed, agx_k_side_firsts; csrc/agx_core.h "compact
wire forms"): a unit uploaded compact and the same unit uploaded with AGX_WIRE_PLAIN=1 leave byte-identical arrays in front of the node sweep (Unit.front(): the derived
hit records are made of d_whits and d_wsides, the tile lists of those) and give the oracle's files and graph — tile-ordered, in file order, with the rows as differences,
in three upload windows, one-shot, and after a second build of the resident unit.  tests/test_wire_codec.py holds the codec itself against every record value on the CPU.

The units (builders of tests/front_units.py) lie in position order in their files, so hit i stands at place i of either upload order and a case can aim at a lane:
  * mixed: 320 hits — mates with several runs on either side and on both (side records, extra words), both strands, mate 2 as the left mate, further hits of a pair (back
    != 0: escapes), reads shorter than the unit's longest (escapes, two of them on lanes 0 and 63 of block 1), other mates 2047 (fits) and 2048 (escapes) positions from
    the left one, a stretch of hits 5 000 positions on that their block's base cannot reach;
  * escapes: every hit's other mate lies 3 000 positions on: every slot escapes, and the unit sends its records as they are;
  * escblock: 320 hits of which the 64 of block 2 are such hits: a block with every slot escaped between compact ones, in a unit that still gains — the device decodes it;
  * big: 1 100 hits, for the byte counts."""
import os

import numpy as np
import pytest

import front_units as FU
import harness as H
import lean_units as LU
from conftest import graph_mismatch

pytestmark = pytest.mark.gpu

FORMS = {"tiled": {}, "file_order": {"AGX_NO_TILED_UPLOAD": "1"}, "rowdiff": {"AGX_ROW_DIFF": "1"}, "windows3": {"AGX_UPLOAD_WINDOWS": "3"}}
SWITCHES = ("AGX_NO_TILED_UPLOAD", "AGX_ROW_DIFF", "AGX_UPLOAD_WINDOWS", "AGX_WIRE_PLAIN", "AGX_REF_RAW", "AGX_TEST_SMALL_CAPS")
ARRAYS = ("vcodes", "runs", "cm_start", "cm", "cm_head", "dhit", "perm", "tile_first", "ckey", "tile_cnt", "tile_off", "tile_recs")
RUNS = "30M2I20M3D48M"


def unit_mixed():
    pairs, more = [], {}
    for i in range(300):
        x, kw = 200 + 9 * i, {}
        if i % 7 == 1:
            kw = dict(cigar=RUNS)
        elif i % 7 == 3:
            kw = dict(other_cigar=RUNS)
        elif i % 7 == 5:
            kw = dict(cigar=RUNS, other_cigar="40S60M")
        if i % 11 == 4:
            kw["left_is_mate2"] = True
        if i in (64, 127, 150, 201):                     # (64, 127: lanes 0 and 63 of block 1 while no later hit of a pair stands in front of them — see `more`)
            pairs.append(FU.P(x, 80, rev=(i % 2 == 1)))
            continue
        gap = 2047 if i == 20 else 2048 if i == 21 else 400
        pairs.append(FU.P(x, gap=gap, rev=(i % 3 == 0), **kw))
        if i in (140, 160, 180, 260):                    # a later hit of the pair, a read length away and further: one dropped, three kept; all with back != 0
            more[i] = [(x + (30 if i == 140 else 300), x + gap + (30 if i == 140 else 300))]
    pairs += [FU.P(9000 + 11 * i, rev=(i % 2 == 0)) for i in range(16)]      # 5 000 positions on, in the last block
    return FU.Case("wire_mixed", "wire", LU.Unit(64 * 160, pairs), 100, [], more=more)


def unit_escapes():
    return FU.Case("wire_escapes", "wire", LU.Unit(64 * 160, [FU.P(200 + 50 * i, gap=3000, rev=(i % 2 == 1)) for i in range(100)]), 100, [])


def unit_escblock():
    pairs = [FU.P(200 + 9 * i, gap=3000 if 128 <= i < 192 else 400, rev=(i % 2 == 1)) for i in range(320)]
    return FU.Case("wire_escblock", "wire", LU.Unit(64 * 160, pairs), 100, [])


def unit_big():
    pairs = [FU.P(200 + 5 * i, rev=(i % 2 == 1), **(dict(cigar=RUNS) if i % 5 == 2 else dict(other_cigar=RUNS) if i % 5 == 4 else {})) for i in range(1100)]
    return FU.Case("wire_big", "wire", LU.Unit(64 * 110, pairs), 100, [])


UNITS = {"mixed": unit_mixed, "escapes": unit_escapes, "escblock": unit_escblock, "big": unit_big}


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
    made = {}

    def get(name):
        if name not in made:
            tmp = FU.write_unit(UNITS[name](), str(tmp_path_factory.mktemp(name)))
            made[name] = (tmp, H.run_oracle(tmp, 0, LU.K, LU.IV, 1, graph=True))
        return made[name]
    return get


def run(agx, tmp, oracle, monkeypatch, env, plain, one_shot=False):
    """One unit through upload, two builds and finish; returns (first front, stats) — (None, stats) one-shot, where nothing can be copied out.  Files and graph against the oracle."""
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    if plain:
        monkeypatch.setenv("AGX_WIRE_PLAIN", "1")
    monkeypatch.setenv("AGX_NO_CACHE", "1")
    d = None
    with agx.Unit(k=LU.K, insert_variation=LU.IV, coverage=1, flags=agx.AGX_FLAG_ONE_SHOT if one_shot else 0, keep_counts=not one_shot) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        st = u.stats()
        if not one_shot:
            d = u.front()
            assert d["w_err"] == 0
            u.build()                        # the resident unit again: nothing is expanded a second time, and nothing may have changed
            d2 = u.front()
            assert front_diff(d, d2) is None
        out = u.finish()
        g = None if one_shot else u.graph()
    for key in ("initial", "pre", "extended"):
        assert out[key] == oracle[key], key
    if g is not None:
        assert graph_mismatch(oracle["graph"], g) is None
    return d, st


def front_diff(a, b):
    if a["ref"] != b["ref"]:
        return "ref"
    for key in ARRAYS:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return key
    for key in ("n_hits", "n_runs", "lookback", "n_entries", "long_count", "n_long", "w_err", "w_status", "tiled", "rows_diffed", "stride", "n_rows"):
        if a[key] != b[key]:
            return key
    if set(np.asarray(a["long_list"]).tolist()) != set(np.asarray(b["long_list"]).tolist()):
        return "long_list"
    return None


@pytest.mark.parametrize("name", list(UNITS))
@pytest.mark.parametrize("form", list(FORMS))
def test_both_wire_forms_leave_the_same_arrays(agx, unit_of, name, form, monkeypatch):
    tmp, oracle = unit_of(name)
    dp, sp = run(agx, tmp, oracle, monkeypatch, FORMS[form], plain=True)
    dc, sc = run(agx, tmp, oracle, monkeypatch, FORMS[form], plain=False)
    print(name, form, "upload_bytes plain", sp["upload_bytes"], "compact", sc["upload_bytes"], "hits", sc["n_hits"])
    assert front_diff(dp, dc) is None
    assert dc["tiled"] == (0 if form == "file_order" else 1)
    assert sp["n_hits"] == sc["n_hits"] and sp["n_nodes"] == sc["n_nodes"]
    if name == "escblock":      # 5 blocks of 528 bytes + 64 escaped records of 16 against 320 records of 16: 1 456 bytes fewer, whatever else the unit sends
        assert sp["upload_bytes"] - sc["upload_bytes"] == 320 * 16 - (5 * 528 + 64 * 16), "the block of escapes did not reach the device as one"
    if name == "mixed":
        assert sc["upload_bytes"] < sp["upload_bytes"], "the unit with escapes of every kind did not cross compact: its escapes never reached the device"


@pytest.mark.parametrize("name", list(UNITS))
def test_one_shot(agx, unit_of, name, monkeypatch):
    tmp, oracle = unit_of(name)
    _, sp = run(agx, tmp, oracle, monkeypatch, {}, plain=True, one_shot=True)
    _, sc = run(agx, tmp, oracle, monkeypatch, {}, plain=False, one_shot=True)
    assert sp["n_nodes"] == sc["n_nodes"] and sc["upload_bytes"] <= sp["upload_bytes"]


@pytest.mark.parametrize("form", list(FORMS))
def test_upload_bytes(agx, unit_of, form, monkeypatch):
    """1 100 hits cross in strictly fewer bytes.  The unit whose every slot escapes: from the format, blocks of escaped slots would be the records + 8 bytes a slot + 16 a
    block, so such a unit sends its records (HitPacker::finish) — at most the plain upload, and with it at most the plain upload plus the 16-byte headers of its blocks."""
    tmp, oracle = unit_of("big")
    _, sp = run(agx, tmp, oracle, monkeypatch, FORMS[form], plain=True, one_shot=True)
    _, sc = run(agx, tmp, oracle, monkeypatch, FORMS[form], plain=False, one_shot=True)
    assert sc["n_hits"] >= 1000 and sc["upload_bytes"] < sp["upload_bytes"]
    saved = sp["upload_bytes"] - sc["upload_bytes"]
    print(form, "big: plain", sp["upload_bytes"], "compact", sc["upload_bytes"], "bytes per hit saved %.2f" % (saved / sc["n_hits"]))
    assert saved >= 4 * sc["n_hits"], "16 -> 8 bytes a slot, 4 more for the two hits in five with a side record, 12 -> 2 a side: at least 4 a hit"
    tmp, oracle = unit_of("escapes")
    _, sp = run(agx, tmp, oracle, monkeypatch, FORMS[form], plain=True, one_shot=True)
    _, sc = run(agx, tmp, oracle, monkeypatch, FORMS[form], plain=False, one_shot=True)
    assert sc["upload_bytes"] <= sp["upload_bytes"] + 16 * ((sc["n_hits"] + 63) // 64)
    assert sc["upload_bytes"] == sp["upload_bytes"], "no side record, every hit escaped: the unit sends what it sent"
