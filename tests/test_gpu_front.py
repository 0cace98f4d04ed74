"""The front of a build on the device — agx_k_expand_runs, agx_k_cm_layout, agx_k_cm_fill, agx_k_expand_codes, agx_k_patch_codes, agx_k_expand_rows, agx_k_expand_ref,
agx_k_patch_ref, agx_k_hit_prep, the scan of the tile histogram, agx_k_tile_fill (its two-tile fast form and agx_tile_fill_general), agx_k_bin_fill and agx_k_tile_sort
(agx_kernels.hip) — as Unit.front() copies it out of HBM, array by array and in full:

  * ref, runs, cm_start, cm, cm_head against the serial executor's; ref also against the file;
  * lookback, perm, tile_first, ckey, tile_cnt, tile_off, long_count, the long list (as a set of file numbers: its order is whatever the atomics gave) and dense_lists
    against the plain model of tests/front_model.py;
  * dhit[i] against the executor's record of hit perm[i], in every field but the row number a_slot — and the device's vcodes row a_slot against the executor's row of
    that hit, over the read's length;
  * every list entry: perm[hit] is the model's e-th file number of that tile, the six geometry words are the executor's lean record of that entry, slot is the a_slot of
    dhit[hit];
  * W_ERR == 0, and after finish() the graph and the three files against the oracle.

Every case of tests/front_units.py runs in every upload form whose switch is read per unit (FORMS), asserts the arm it is there for (on the executor's records here, as
the CPU twin tests/test_front_cases.py does, and on the device through the equality of its counts, lists and form flags with the model's), and builds a second time on the
resident unit — nothing is expanded again — after which every array must be what it was.

Left unspecified: the bytes of a vcodes row from the read's length up to the stride (the two sides pad rows to different strides: a multiple of 4 here, of 16 in the
executor); in the tile-ordered form the rows of skipped hits (the executor gives a skipped hit no row); the order of the long list.

AGX_SCAN_LEGACY (the three-launch scan) is read once when the library loads and cannot be switched inside a test process: it is not covered here."""
import os

import numpy as np
import pytest

import front_units as FU
import harness as H
import lean_units as LU
from conftest import graph_mismatch
from hostsim import sim

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in FU.cases()}
FORMS = {"tiled": {}, "file_order": {"AGX_NO_TILED_UPLOAD": "1"}, "rowdiff_tiled": {"AGX_ROW_DIFF": "1"}, "rowdiff_file_order": {"AGX_ROW_DIFF": "1", "AGX_NO_TILED_UPLOAD": "1"},
         "ref_raw": {"AGX_REF_RAW": "1"}, "windows3": {"AGX_UPLOAD_WINDOWS": "3"}, "rowdiff_windows3": {"AGX_ROW_DIFF": "1", "AGX_UPLOAD_WINDOWS": "3"}}
SWITCHES = ("AGX_NO_TILED_UPLOAD", "AGX_ROW_DIFF", "AGX_REF_RAW", "AGX_UPLOAD_WINDOWS", "AGX_TEST_SMALL_CAPS")
ARRAYS = ("ref", "vcodes", "runs", "cm_start", "cm", "cm_head", "dhit", "perm", "tile_first", "ckey", "tile_cnt", "tile_off", "tile_recs")
GEOMETRY = ("qoff1", "boff1", "qoff2", "boff2", "lenjs", "geo")


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
    """Writes a case's unit, dumps the executor's front, asserts the case's arm on it and runs the oracle, once per module."""
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            tmp = FU.write_unit(case, str(tmp_path_factory.mktemp(name)))
            s = sim.run(tmp, 0, LU.K, LU.IV, 1, front=True)
            v = FU.View(case, s["front"], tmp)
            FU.check_arms(case, v)
            made[name] = (tmp, v, H.run_oracle(tmp, 0, LU.K, LU.IV, 1, graph=True))
        return made[name]
    return get


def first_diff(got, want):
    """Index of the first element in which two arrays (plain or structured) differ, with the field's name; None if they are equal."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    if got.dtype.names:
        worst = None
        for name in got.dtype.names:
            ne = np.nonzero(got[name] != want[name])[0]
            if len(ne) and (worst is None or ne[0] < worst[0]):
                worst = (int(ne[0]), name, got[name][ne[0]], want[name][ne[0]])
        return None if worst is None else "[%d].%s = %s, expected %s" % worst
    ne = np.argwhere(got != want)
    return None if not len(ne) else "%s = %s, expected %s" % (tuple(int(x) for x in ne[0]), got[tuple(ne[0])], want[tuple(ne[0])])


def front_mismatch(v, d, stats):
    """First difference between the device's front `d` and the executor + model of View `v`, as text that names the array, the index and the hit or tile; None if there is none."""
    f, m = v.f, v.m
    for key in ("n_pos", "n_hits", "n_runs", "n_cm", "n_tiles"):
        if int(d[key]) != int(f[key]):
            return "%s = %d, expected %d" % (key, d[key], f[key])
    if d["w_err"] != 0:
        return "W_ERR = %d" % d["w_err"]
    if d["ref"] != f["ref"] or d["ref"][:int(stats["n_ref"])] != v.file_ref:
        i = next(i for i in range(v.n_pos) if d["ref"][i:i + 1] != f["ref"][i:i + 1] or (i < len(v.file_ref) and d["ref"][i:i + 1] != v.file_ref[i:i + 1]))
        return "ref[%d] = %r, expected %r" % (i, d["ref"][i:i + 1], f["ref"][i:i + 1])
    for key in ("runs", "cm_start", "cm", "cm_head"):
        x = first_diff(d[key], f[key])
        if x is not None:
            return "%s%s (against the executor)" % (key, x)
    if d["lookback"] != m["lookback"]:
        return "lookback = %d, expected %d" % (d["lookback"], m["lookback"])
    nt = m["n_tiles"]
    for key, want in (("tile_cnt", m["tile_cnt"]), ("tile_off", m["tile_off"]), ("perm", m["order"]), ("tile_first", m["tile_first"]), ("ckey", m["ckey"])):
        x = first_diff(d[key].astype(np.int64), want)
        if x is not None:
            return "%s%s (against the model; %s)" % (key, x, "index = tile of %d" % nt if key.startswith("tile") else "index = place in the device's order")
    if d["long_count"] != m["long_count"] or d["n_long"] != min(m["long_count"], 1024):
        return "long_count = %d (%d listed), expected %d" % (d["long_count"], d["n_long"], m["long_count"])
    perm = d["perm"].astype(np.int64)
    longs = perm[d["long_list"].astype(np.int64)].tolist() if d["n_long"] else []
    if len(set(longs)) != len(longs) or not set(longs) <= m["long_hits"] or (m["long_count"] <= 1024 and set(longs) != m["long_hits"]):
        return "long list: hits %s, expected %s" % (sorted(set(longs) ^ m["long_hits"])[:8], "those of the model")
    if stats["dense_lists"] != m["dense_lists"]:
        return "dense_lists = %d, expected %d" % (stats["dense_lists"], m["dense_lists"])
    # the derived records, in the device's order, against the executor's in file order
    dh, eh = d["dhit"], f["dhit"][perm]
    for name in dh.dtype.names:
        if name == "a_slot":
            continue
        ne = np.nonzero(dh[name] != eh[name])[0]
        if len(ne):
            return "dhit[%d].%s = %d, expected %d (hit %d of the file)" % (ne[0], name, dh[name][ne[0]], eh[name][ne[0]], perm[ne[0]])
    kept = np.nonzero(m["kept"][perm])[0]
    if len(kept):
        if int(dh["a_slot"][kept].max()) >= d["n_rows"]:
            return "dhit.a_slot = %d with %d rows" % (dh["a_slot"][kept].max(), d["n_rows"])
        width = min(d["stride"], f["stride"])
        rows_d, rows_e = d["vcodes"][dh["a_slot"][kept], :width], f["vcodes"][eh["a_slot"][kept], :width]
        bad = (rows_d != rows_e) & (np.arange(width)[None, :] < dh["len"][kept].astype(np.int64)[:, None])
        if bad.any():
            r, c = (int(x) for x in np.argwhere(bad)[0])
            return "vcodes[%d][%d] = %d, expected %d (row of the hit at place %d, hit %d of the file)" % (dh["a_slot"][kept[r]], c, rows_d[r, c], rows_e[r, c], kept[r], perm[kept[r]])
    # the lists
    recs, er = d["tile_recs"], f["tile_recs"]
    if len(recs) != len(m["entry_hit"]):
        return "%d list entries, expected %d" % (len(recs), len(m["entry_hit"]))
    if len(recs):
        if int(recs["hit"].max()) >= len(perm):
            e = int(np.argmax(recs["hit"]))
            return "tile_recs[%d].hit = %d with %d hits (tile %d)" % (e, recs["hit"][e], len(perm), m["entry_tile"][e])
        ne = np.nonzero(perm[recs["hit"].astype(np.int64)] != m["entry_hit"])[0]
        if len(ne):
            e = int(ne[0])
            return "tile_recs[%d] (tile %d, entry %d of its list) is hit %d of the file, expected hit %d" % (e, m["entry_tile"][e], e - m["tile_off"][m["entry_tile"][e]], perm[recs["hit"][e]], m["entry_hit"][e])
        for name in GEOMETRY:
            ne = np.nonzero(recs[name] != er[name])[0]
            if len(ne):
                e = int(ne[0])
                return "tile_recs[%d].%s = %#x, expected %#x (tile %d, hit %d of the file)" % (e, name, recs[name][e], er[name][e], m["entry_tile"][e], m["entry_hit"][e])
        ne = np.nonzero(recs["slot"] != dh["a_slot"][recs["hit"].astype(np.int64)])[0]
        if len(ne):
            e = int(ne[0])
            return "tile_recs[%d].slot = %d, expected the a_slot %d of its hit (tile %d, hit %d of the file)" % (e, recs["slot"][e], dh["a_slot"][recs["hit"][e]], m["entry_tile"][e], m["entry_hit"][e])
    return None


def same_front(a, b):
    """A rebuilt front against the first one: every array, the counts and the words; the long list as a set."""
    for key in ARRAYS:
        x = (None if a[key] == b[key] else "differs") if key == "ref" else first_diff(b[key], a[key])
        if x is not None:
            return "%s%s after the second build" % (key, x if key != "ref" else " differs")
    for key in ("lookback", "n_entries", "long_count", "n_long", "w_err", "w_status", "tiled", "rows_diffed", "ref_packed", "stride", "n_rows"):
        if a[key] != b[key]:
            return "%s = %d after the second build, was %d" % (key, b[key], a[key])
    if a["long_count"] <= a["n_long"] and set(a["long_list"].tolist()) != set(b["long_list"].tolist()):      # (beyond 1 024 long hits the list holds whichever 1 024 the atomics let in)
        return "the long list differs after the second build"
    return None


# (the case varies fastest: consecutive units then differ in size and content, so a block of HBM that the library's cache hands to the next unit does not already hold,
#  from the same case in another form, the very bytes a kernel should have written)
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("form", list(FORMS))
def test_front_matches_the_executor_and_the_model(agx, unit_of, name, form, monkeypatch):
    case = CASES[name]
    tmp, v, o = unit_of(name)
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in FORMS[form].items():
        monkeypatch.setenv(key, val)
    with agx.Unit(k=LU.K, insert_variation=LU.IV, coverage=1, keep_counts=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        d, st = u.front(), u.stats()
        assert front_mismatch(v, d, st) is None
        # the forms the unit used
        env = FORMS[form]
        assert d["tiled"] == (0 if "AGX_NO_TILED_UPLOAD" in env else 1)
        assert d["ref_packed"] == (0 if "AGX_REF_RAW" in env else case.device.get("ref_packed", 1))
        # (the windows are the FIRST attempt's: a build that had to repeat — long_1025 — converges on an attempt that sweeps the resident rows in one piece)
        assert d["swept_windows"] == (3 if "AGX_UPLOAD_WINDOWS" in env and st["build_attempts"] == 1 else 1) and d["w_status"] & 16 == 0
        if "AGX_ROW_DIFF" not in env:
            assert d["rows_diffed"] == 0 and st["rows_by_reference"] == 0
        elif case.row_diff:
            assert d["rows_diffed"] == 1 and 0 < st["rows_by_reference"] < d["n_rows"], "rows by reference: %d of %d" % (st["rows_by_reference"], d["n_rows"])
        for key, want in case.device.items():
            got = d[key] if key in d else st[key]
            assert want(got) if callable(want) else got == want, "%s = %s" % (key, got)
        # a second build on the resident unit
        u.build()
        d2 = u.front()
        assert same_front(d, d2) is None
        assert d2["swept_windows"] == 1 and front_mismatch(v, d2, u.stats()) is None
        out = u.finish()
        g = u.graph()
    for key in ("initial", "pre", "extended"):
        assert out[key] == o[key], key
    assert graph_mismatch(o["graph"], g) is None


def test_rowdiff_windows3_sends_rows_as_differences_and_sweeps_three_windows(agx, unit_of, monkeypatch):
    """The form counts only where a unit keeps both: the encoder drops the differences where they gain nothing, and then the form is windows3 again.  The rows_* cases keep
    them (row_diff: asserted per case above, as under rowdiff_tiled); rows_130 has rows in all three windows — pieces that begin at blocks 0, 1 and 2 of the stream."""
    tmp, v, o = unit_of("rows_130")
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in FORMS["rowdiff_windows3"].items():
        monkeypatch.setenv(key, val)
    with agx.Unit(k=LU.K, insert_variation=LU.IV, coverage=1, keep_counts=True) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        d = u.front()
        assert d["rows_diffed"] == 1 and d["swept_windows"] == 3 and d["tiled"] == 1
        assert front_mismatch(v, d, u.stats()) is None


def test_front_is_refused_where_the_arrays_are_not_there(agx, unit_of):
    tmp, v, o = unit_of("hist_spans")
    with agx.Unit(k=LU.K, insert_variation=LU.IV, coverage=1) as u:
        u.load_files(tmp, 0)
        u.upload()
        with pytest.raises(agx.AgxError) as e:
            u.front()
        assert e.value.code == agx.AGX_E_ARG and "not built" in e.value.msg
        u.build()
        assert front_mismatch(v, u.front(), u.stats()) is None
        u.download()
        for after in ("download", "trim", "release"):
            if after == "trim":
                u.trim()
            if after == "release":
                u.release()
            with pytest.raises(agx.AgxError) as e:
                u.front()
            assert e.value.code == agx.AGX_E_ARG and "not built" in e.value.msg, after
        u.upload()
        u.build()
        assert front_mismatch(v, u.front(), u.stats()) is None
        out = u.finish()
    for key in ("initial", "pre", "extended"):
        assert out[key] == o[key], key
    with agx.Unit(k=LU.K, insert_variation=LU.IV, coverage=1, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        u.load_files(tmp, 0)
        u.upload()
        u.build()
        with pytest.raises(agx.AgxError) as e:
            u.front()
        assert e.value.code == agx.AGX_E_ARG and "one-shot" in e.value.msg
        out = u.finish()
    for key in ("initial", "pre", "extended"):
        assert out[key] == o[key], key
