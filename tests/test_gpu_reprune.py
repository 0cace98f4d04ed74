"""agx_unit_reprune on the MI355X (-m gpu): a built unit re-pruned at another coverage must be, in everything a caller can observe, the unit a build at that coverage
leaves.  So after every reprune: the walk graph in both download forms, with every record through the fetch path, against the model of tests/walk_model.py on the oracle's
graph at the new threshold; finish() against the oracle's three files at the new threshold; the counts in stats() against the model.  On two generated units through every
threshold in an order that goes up and down (the sparse record table must grow on the way down), on the hand-made units of tests/test_gpu_walk_graph.py, with every
capacity starting too small, beside the exports (whole export = region export at the new coverage; exports at an explicit threshold and agx_unit_graph untouched), with
kept paths, followed by a rebuild and by a fresh upload, on a one-shot unit, beside another unit's builds on the same device, and the calls that are refused.
tests/test_reprune_lane.py checks the lane function of the kernel on the CPU."""
import os
import threading

import numpy as np
import pytest

import edge_units as EU
import harness as H
import lean_units as LU
import path_model as PM
import unitig_region_model as URM
import walk_model as WM
import walk_units as WU
from test_gpu_parity import CONFIGS

pytestmark = pytest.mark.gpu

ORDER = (1 << 30, 0, 8, 1, 20, 3, 5)      # every threshold of the issue, up and down; the last one is the units' own coverage
KEYS = ("initial", "pre", "extended")
CASES = {c.name: c for c in WU.cases()}
OTHER = {"edge:" + c.name: c for c in EU.cases() if c.overflow or c.windows}
OTHER["lean:contimers"] = LU.case_contimers()


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


class Ref:
    """One unit's files, its graph dump and the oracle's outputs per threshold (each made once per module, never changed)."""

    def __init__(self, tmp, k, iv, cov):
        self.tmp, self.k, self.iv, self.cov = tmp, k, iv, cov
        self.g = H.run_oracle(tmp, 0, k, iv, cov, graph=True)["graph"]
        self.n = int(self.g["n_pos"])
        self._at, self._model = {}, {}

    def at(self, c):
        if c not in self._at:
            self._at[c] = H.run_oracle(self.tmp, 0, self.k, self.iv, c)
        return self._at[c]

    def model(self, c):
        if c not in self._model:
            self._model[c] = WM.build(self.g, c)
        return self._model[c]

    def streams(self):
        return self.n >= 4096


@pytest.fixture(scope="module")
def ref_of(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            if isinstance(name, int):
                cfg = next(c for c in CONFIGS if c["seed"] == name)
                run = H.synth(str(tmp_path_factory.mktemp("run%d" % name) / "run"), sam_seq=0, **cfg)
                meta = H.read_meta(run)
                made[name] = Ref(os.path.join(run, "tmp"), meta["k"], meta["insert_variation"], meta["coverage"])
            else:
                case = CASES.get(name) or OTHER[name]
                tmp = WU.write_unit(case.unit, str(tmp_path_factory.mktemp(name.replace(":", "_"))))
                made[name] = Ref(tmp, LU.K, getattr(case, "iv", LU.IV), getattr(case, "coverage", 1))
        return made[name]
    return get


def unit_of(agx, r, cov=None, build=True, **kw):
    kw.setdefault("keep_counts", True)
    u = agx.Unit(k=r.k, insert_variation=r.iv, coverage=r.cov if cov is None else cov, **kw)
    u.load_files(r.tmp, 0)
    u.upload()
    if build:
        u.build()
    return u


def same_outputs(out, want):
    for key in KEYS:
        assert out[key] == want[key], key


def check_unit_at(u, r, c, streamed=False, dump=True):
    """The unit is what a build at coverage c leaves: walk graph (one download form), outputs, counts.  Returns (outputs, stats)."""
    m = r.model(c)
    if dump:
        assert WM.mismatch(m, u.walk_graph(streamed=streamed, all_node=True)) is None, c
    out = u.finish()
    same_outputs(out, r.at(c))
    st = u.stats()
    assert (st["n_walk_ids"], st["n_special"]) == (m["n_ids"], m["n_special"]), c
    return out, st


# ---- 1. every threshold, any order ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [201, 203])
def test_every_threshold_in_any_order(agx, ref_of, seed, monkeypatch):
    r = ref_of(seed)
    assert r.cov == 5 and r.streams()
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    attempts, pres = [], []
    with unit_of(agx, r) as u:
        first, _ = check_unit_at(u, r, r.cov)
        for i, c in enumerate(ORDER):
            u.reprune(c)
            assert u.params.coverage == c
            attempts.append(u.stats()["reprune_attempts"])
            out, st = check_unit_at(u, r, c, streamed=bool(i & 1))
            assert st["ms_reprune"] > 0
            pres.append(out["pre"])
        assert out == first                                  # back at the unit's own coverage: its outputs from before the first reprune
    assert len(set(pres)) == len(ORDER), "the seven thresholds give seven different pre-extended files"
    sides = [r.model(c)["n_ids"] - r.n for c in ORDER]
    print("seed %d: side ids %s, special ids %s, reprune_attempts %s" % (seed, sides, [r.model(c)["n_special"] for c in ORDER], attempts))
    assert all(a in (1, 2) for a in attempts)
    if seed == 203:
        assert 2 in attempts, "lowering the threshold from 2^30 to 0 nearly doubles the special ids: the sparse record table must have grown"


# ---- 2. hand-made units -------------------------------------------------------------------------------------------------------------------

def down_up_and_back(agx, r, **kw):
    attempts = []
    with unit_of(agx, r, **kw) as u:
        first, _ = check_unit_at(u, r, r.cov)
        for i, c in enumerate((0, 1 << 30, r.cov)):
            u.reprune(c)
            attempts.append(u.stats()["reprune_attempts"])
            out, _ = check_unit_at(u, r, c, streamed=r.streams() and bool(i & 1))      # (units too small for a streamed dump: the whole form only)
        assert out == first
    return attempts


@pytest.mark.parametrize("name", list(CASES) + list(OTHER))
def test_hand_made_units(agx, ref_of, name, monkeypatch):
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    down_up_and_back(agx, ref_of(name))


# ---- 3. small capacities --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.small_caps])
def test_hand_made_units_with_every_capacity_too_small(agx, ref_of, name, monkeypatch):
    monkeypatch.setenv("AGX_TEST_SMALL_CAPS", "1")
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    down_up_and_back(agx, ref_of(name))


def test_generated_unit_from_20_down_to_0_with_small_capacities(agx, ref_of, monkeypatch):
    r = ref_of(203)
    monkeypatch.setenv("AGX_TEST_SMALL_CAPS", "1")
    monkeypatch.setenv("AGX_STREAM_PIECES", "2")
    attempts = []
    with unit_of(agx, r, cov=20) as u:
        assert u.stats()["build_attempts"] > 1
        check_unit_at(u, r, 20)
        for i, c in enumerate((8, 5, 3, 1, 0)):
            u.reprune(c)
            attempts.append(u.stats()["reprune_attempts"])
            check_unit_at(u, r, c, streamed=bool(i & 1))
    assert max(attempts) > 1, attempts


# ---- 4. exports agree -----------------------------------------------------------------------------------------------------------------------

def test_exports_follow_the_reprune_and_explicit_thresholds_do_not(agx, ref_of):
    r = ref_of(201)
    g, n, ref = r.g, r.n, bytes(r.g["pos_nuc"])
    with unit_of(agx, r) as u:
        window = u.gfa(0, region=(100, 5000), min_coverage=1)
        assert window == URM.region_gfa(g, 100, 5000, 1, ref, 0)
        graph = u.graph()
        held = u.stats()["device_bytes"]
        for c in (0, 3, 1 << 30):
            u.reprune(c)
            st = u.stats()
            assert st["device_bytes"] == held or st["reprune_attempts"] == 2
            held = st["device_bytes"]
            whole = u.gfa(0)
            assert whole == URM.region_gfa(g, 0, n, c, ref, 0), c
            assert whole == u.gfa(0, region=(0, n), min_coverage=c), c
            assert u.gfa(0, region=(100, 5000)) == URM.region_gfa(g, 100, 5000, c, ref, 0), c      # no threshold: the unit's own coverage, which is now c
            assert u.gfa(0, region=(100, 5000), min_coverage=1) == window, c
            again = u.graph()
            assert sorted(again) == sorted(graph)
            for key, v in graph.items():
                assert np.array_equal(again[key], v), (c, key)


# ---- 5. paths ---------------------------------------------------------------------------------------------------------------------------------

def test_kept_paths_are_dropped_and_made_again_at_the_new_coverage(agx, ref_of):
    r = ref_of(201)
    g, n, ref = r.g, r.n, bytes(r.g["pos_nuc"])
    with unit_of(agx, r, keep_paths=True) as u:
        u.finish()
        assert len(u.walk_paths()["rec_len"]) > 0
        u.reprune(3)
        with pytest.raises(agx.AgxError) as e:
            u.walk_paths()
        assert e.value.code == agx.AGX_E_ARG
        t = u.unitigs(id_map=True)
        out = u.finish()
        w = u.walk_paths()
    wm = r.model(3)
    mu, es, er = PM.id_map(g, 3, 0, n, 3, ref, wm)
    assert (t["id_map"]["n_pos"], t["id_map"]["n_ids"]) == (mu["id_map"]["n_pos"], mu["id_map"]["n_ids"])
    for f in ("id_first", "id_last", "seg", "rank_first"):
        assert np.array_equal(t["id_map"][f], mu["id_map"][f]), f
    same_outputs(out, r.at(3))
    assert [len(x) for x in PM.fasta_records(out["pre"])] == w["rec_len"].tolist()
    text = agx.gfa_paths(t, w, 0)
    assert text and text == PM.paths_gfa(mu, es, er, w, 0)


# ---- 6. what follows a reprune ------------------------------------------------------------------------------------------------------------------

def test_a_rebuild_and_a_fresh_upload_keep_the_new_coverage(agx, ref_of):
    r = ref_of(203)
    with unit_of(agx, r) as u:
        u.reprune(8)
        u.build()
        check_unit_at(u, r, 8)
        u.upload()
        u.build()
        check_unit_at(u, r, 8)
        assert u.params.coverage == 8


def test_one_shot_unit_is_repruned_before_its_download_only(agx, ref_of):
    r = ref_of(203)
    with unit_of(agx, r, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        u.reprune(8)
        check_unit_at(u, r, 8, dump=False)                 # (a one-shot unit refuses the dump)
        with pytest.raises(agx.AgxError) as e:
            u.reprune(3)
        assert e.value.code == agx.AGX_E_ARG and "one-shot" in e.value.msg
        assert u.params.coverage == 8
        same_outputs(u.finish(), r.at(8))                  # still usable


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------

def refused(agx, u, c, word=None):
    before = u.params.coverage
    with pytest.raises(agx.AgxError) as e:
        u.reprune(c)
    assert e.value.code == agx.AGX_E_ARG
    if word:
        assert word in e.value.msg, e.value.msg
    assert u.params.coverage == before


def test_refusals_leave_the_unit_usable(agx, ref_of):
    r = ref_of(201)
    with unit_of(agx, r, keep_counts=False) as u:
        refused(agx, u, 3, "KEEP_COUNTS")
        same_outputs(u.finish(), r.at(r.cov))
    with unit_of(agx, r, build=False) as u:
        refused(agx, u, 3, "not built")
        u.build()
        for c in (1 << 31, -1, 1 << 32):
            refused(agx, u, c)
        same_outputs(u.finish(), r.at(r.cov))
        u.download()
        u.trim()
        refused(agx, u, 3, "trim")
        same_outputs(u.finish(), r.at(r.cov))
        u.release()
        refused(agx, u, 3, "release")
        u.upload()
        u.build()
        u.reprune(3)
        same_outputs(u.finish(), r.at(3))


# ---- 8. beside another unit's builds ----------------------------------------------------------------------------------------------------------------

def test_reprune_beside_another_units_builds(agx, ref_of):
    a, b = ref_of(201), ref_of(203)
    for c in ORDER:
        a.at(c)
    b.at(b.cov)
    done, errors, rounds = threading.Event(), [], [0]

    def sweep():
        try:
            with unit_of(agx, a) as u:
                for c in ORDER:
                    u.reprune(c)
                    same_outputs(u.finish(), a.at(c))
        except Exception as e:      # noqa: BLE001  (reported by the main thread)
            errors.append(e)
        finally:
            done.set()

    def rebuild():
        try:
            with unit_of(agx, b, keep_counts=False) as u:
                while True:
                    same_outputs(u.finish(), b.at(b.cov))
                    rounds[0] += 1
                    if done.is_set():
                        break
                    u.build()
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=sweep), threading.Thread(target=rebuild)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert rounds[0] >= 1
