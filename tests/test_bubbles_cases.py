"""The host-only twin of the bubbles (agx_unitigs_bubbles, through libagx.so: the lane function agx_bubble_class that the kernels call, and the row writer) on the CPU,
against tests/bubbles_model.py applied to the region model's table of the oracle's graph: the hand table of tests/bubbles_units.py, every case of tests/unitig_units.py
on its named windows, the generated units seed201 and seed203 whole at thresholds 0 and 5, and the hand-made units of tests/bubbles_units.py.  Every comparison is
integer equality.  The kernels themselves run the same units in tests/test_gpu_bubbles.py."""
import os

import numpy as np
import pytest

import bubbles_model as BM
import bubbles_units as BU
import harness as H
import lean_units as LU
import unitig_region_model as R
import unitig_units as UU
import walk_units as WU
from test_gpu_parity import CONFIGS

UNITIG_CASES = {c.name: c for c in UU.cases()}
UNITS = {u.name: u for u in BU.units()}
# forks by class of the generated units, whole window: (segments, links, forks, bubbles, TIP, NESTED, SINKS_DIFFER, SINK_SHARED) at threshold 0, and the bubbles at 5
SEEDS = {201: ((2198, 3231, 1060, 922, 29, 55, 48, 6), 884), 203: ((6658, 7949, 2152, 400, 462, 378, 884, 28), 270)}


@pytest.fixture(scope="module")
def A(built):
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    return A


def fake_support(t):
    return (np.arange(len(t["link_from"]), dtype=np.int64) * 7 + 1).astype(np.uint32)


def check(A, t, what, max_nodes=None, support=False):
    """the twin's answer for table t is the model's; returns the model's"""
    sup = fake_support(t) if support else None
    want = BM.bubbles(t, sup, max_nodes)
    got = A.unitigs_bubbles(t, sup, max_nodes)
    x = BM.mismatch(got, want)
    assert x is None, "%s (max_nodes %s): %s" % (what, max_nodes, x)
    assert A.bubbles_tsv(got, 3) == BM.tsv(want, 3), what
    return want


def test_hand_table(A):
    t, sup = BU.hand_table()
    for mx in (None, 0, 1, BU.HAND_LONGEST - 1, BU.HAND_LONGEST, BU.HAND_LONGEST + 1):
        for s in (None, sup):
            got = A.unitigs_bubbles(t, s, mx)
            assert BM.mismatch(got, BM.bubbles(t, s, mx)) is None, (mx, s is not None)
    got = A.unitigs_bubbles(t, sup)
    assert {f: int(got[f]) for f in BM.TOTALS} == BU.HAND_TOTALS
    for f, v in BU.HAND_ALL.items():
        assert (bytes(got[f]) if f == "seq" else got[f].tolist()) == v, f
    assert A.bubbles_tsv(got, 7) == BU.HAND_TSV


def test_broken_tables_are_refused(A):
    t, sup = BU.hand_table()
    for field, i, v in (("link_to", 4, 26), ("link_from", 3, 26), ("link_from", 5, 0), ("n_nodes", 2, 6)):
        bad = {k: (list(x) if isinstance(x, list) else x) for k, x in t.items()}
        bad[field][i] = v
        with pytest.raises(A.AgxError):
            A.unitigs_bubbles(bad, sup)
    with pytest.raises(A.AgxError):
        A.unitigs_bubbles(t, sup[:-1])


@pytest.fixture(scope="module")
def graphs(built, tmp_path_factory):
    made = {}

    def get(kind, name):
        if (kind, name) not in made:
            if kind == "seed":
                cfg = next(c for c in CONFIGS if c["seed"] == name)
                run = H.synth(str(tmp_path_factory.mktemp("run%d" % name) / "run"), sam_seq=0, **cfg)
                meta = H.read_meta(run)
                g = H.run_oracle(os.path.join(run, "tmp"), 0, meta["k"], meta["insert_variation"], meta["coverage"], graph=True)["graph"]
            else:
                u = UNITIG_CASES[name] if kind == "unitig" else UNITS[name]
                tmp = WU.write_unit(u.unit, str(tmp_path_factory.mktemp(name)))
                g = H.run_oracle(tmp, 0, LU.K, u.iv, u.coverage, graph=True)["graph"]
            made[(kind, name)] = g
        return made[(kind, name)]
    return get


@pytest.mark.parametrize("name", list(UNITIG_CASES))
def test_unitig_cases(A, graphs, name):
    g, case = graphs("unitig", name), UNITIG_CASES[name]
    ref, forks = bytes(g["pos_nuc"]), 0
    for i, (lo, hi, cov) in enumerate(case.windows):
        t = R.region_unitigs(g, lo, hi, cov, ref)
        b = check(A, t, "%s: window [%d, %d) at %d" % (name, lo, hi, cov), support=i % 2 == 0)
        forks += b["n_forks"]
        if name == "branch_lanes":
            assert (b["n_forks"], b["n_bubbles_all"]) == (1, 1) and (len(t["head_pos"]), len(t["link_from"])) in ((4, 3), (6, 5)), (lo, hi, cov, len(t["head_pos"]))
    if name in ("branch_lanes", "fans"):
        assert forks > 0
    if name == "fans":
        b = check(A, R.region_unitigs(g, 0, int(g["n_pos"]), 0, ref), "fans, whole at 0", max_nodes=1)
        assert (b["n_segs"], b["n_links"], b["n_forks"], b["n_bubbles_all"], b["n_nested"], b["n_sinks_differ"]) == (63, 118, 10, 0, 1, 9)


@pytest.mark.parametrize("seed", list(SEEDS))
def test_generated_units(A, graphs, seed):
    g = graphs("seed", seed)
    ref, n = bytes(g["pos_nuc"]), int(g["n_pos"])
    t0 = R.region_unitigs(g, 0, n, 0, ref)
    b0 = check(A, t0, "seed%d at 0" % seed, support=True)
    at0, bubbles5 = SEEDS[seed]
    assert tuple(b0[f] for f in ("n_segs", "n_links", "n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared")) == at0
    b5 = check(A, R.region_unitigs(g, 0, n, 5, ref), "seed%d at 5" % seed)
    assert b5["n_bubbles_all"] == bubbles5
    k = np.diff(b0["br_off"]).tolist()
    direct = [sum(1 for r in range(b0["br_off"][i], b0["br_off"][i + 1]) if b0["br_pos"][r] == BM.NONE) for i in range(len(k))]
    if seed == 201:
        assert (k.count(2), k.count(3)) == (921, 1) and direct.count(1) == 894 and direct.count(0) == 28 and b0["longest_branch"] == 96
        assert sum(1 for i in range(len(k)) if direct[i] == 0 and k[i] == 2) == 28, "substitutions: two segment branches"
    else:
        assert (k.count(2), k.count(3), k.count(12)) == (392, 7, 1) and b0["n_segs"] > 4096, "the scans take a second level"
    for mx in (0, 1, b0["longest_branch"] - 1, b0["longest_branch"]):
        check(A, t0, "seed%d at 0" % seed, max_nodes=mx, support=True)


@pytest.mark.parametrize("name", list(UNITS))
def test_hand_made_units(A, graphs, name):
    g, u = graphs("unit", name), UNITS[name]
    ref, seen = bytes(g["pos_nuc"]), {}
    for lo, hi, cov in u.windows:
        hi = min(hi, int(g["n_pos"]))
        t = R.region_unitigs(g, lo, hi, cov, ref)
        seen[(lo, hi, cov)] = (check(A, t, "%s: window [%d, %d) at %d" % (name, lo, hi, cov), support=True), t)
        check(A, t, "%s: window [%d, %d) at %d" % (name, lo, hi, cov), max_nodes=0)
    for what, w, fn in u.want:
        b, t = seen[(w[0], min(w[1], int(g["n_pos"])), w[2])]
        assert fn(b, t), "%s: window %s: %s; the model has %s" % (name, w, what, {f: b[f] for f in BM.TOTALS})
