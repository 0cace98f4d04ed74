"""Paths on the MI355X (-m gpu): the id map of Unit.unitigs(id_map=True) exactly against the path model on the oracle's graph (tests/path_model.py), the stretches of
Unit.walk_paths() against the oracle-derived walk model (tests/walk_model.py) and the record's own bases, the P lines of gfa_paths() byte for byte against the model's, and
every path's segments spelled out against pre_extended — on every hand-made walk unit, a pile of 180 variants and two generated configurations; windows whose edges sit
around the wavefront and block sizes; thresholds below and above the build's coverage; the same stretches and text whatever the walkers, the download's form and the kind
of unit; nothing else disturbed; the calls that are refused."""
import os
import random

import numpy as np
import pytest

import harness as H
import lean_units as LU
import path_model as PM
import unitig_model as M
import walk_model as WM
import walk_units as WU
from conftest import write_pileup_unit
from test_gpu_parity import CONFIGS

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in WU.cases()}
assert {c.group for c in CASES.values()} == set(WU.GROUPS)
TABLE = ("head_pos", "head_var", "n_nodes", "last_pos", "coverage", "seq_off", "link_from", "link_to")
RUNS = ("id_first", "id_last", "seg", "rank_first")
STRETCHES = ("rec_len", "st_off", "id_first", "id_last", "base_off", "joined")


@pytest.fixture(scope="module")
def agx():
    import aligngraph_amd as A
    if not os.path.exists(A.LIB_PATH):
        from aligngraph_amd import build as B
        B.build()
    assert A.device_count() > 0, "no HIP device: the gpu tests must run on the MI355X box"
    return A


def built_unit(agx, tmp, unit, k, iv, cov, flags=0, keep_paths=True, keep_counts=True):
    u = agx.Unit(k=k, insert_variation=iv, coverage=cov, keep_counts=keep_counts, keep_paths=keep_paths, flags=flags)
    u.load_files(tmp, unit)
    u.upload()
    u.build()
    return u


def same_table(a, b):
    return all(np.array_equal(a[f], b[f]) for f in TABLE) and bytes(a["seq"]) == bytes(b["seq"])


def same_map(got, want):
    assert (got["n_pos"], got["n_ids"]) == (want["n_pos"], want["n_ids"])
    for f in RUNS:
        assert np.array_equal(got[f], want[f]), f


def same_stretches(a, b):
    return all(np.array_equal(a[f], b[f]) for f in STRETCHES)


def check_stretches(w, pre, wm):
    """The stretches against the walk model: a record's bases there are the ids' bases, every id inside a stretch steps to the next one by the cont edge, a joined boundary is an
    edge.  Returns the records' sequences."""
    recs = PM.fasta_records(pre)
    assert len(recs) == len(w["rec_len"]) and [len(r) for r in recs] == w["rec_len"].tolist()
    st_off = w["st_off"].tolist()
    assert st_off[0] == 0 and st_off[-1] == len(w["id_first"])
    first, last, base, joined = (w[k].tolist() for k in ("id_first", "id_last", "base_off", "joined"))
    edges = []
    for r, rec in enumerate(recs):
        for i in range(st_off[r], st_off[r + 1]):
            a, b, o = first[i], last[i], base[i]
            assert a <= b < wm["n_ids"]
            assert rec[o:o + b - a + 1] == wm["str"][a:b + 1], (r, i)
            assert wm["has"][a:b + 1].all() and wm["cont"][a:b].all(), (r, i)
            if i == st_off[r]:
                assert not joined[i]
            else:
                end = base[i - 1] + last[i - 1] - first[i - 1] + 1
                assert o >= end and bool(joined[i]) == (o == end), (r, i)
                if joined[i]:
                    edges.append((last[i - 1] << 32) | a)
    assert np.isin(np.array(edges, np.int64), wm["edges"]).all()
    return recs


def check_path_bases(text, t, recs, unit):
    """Every P line spelled out: its segments' bases, without the first fs and behind the last segment's node ls, are the record's bases from the path's first base on."""
    name = {b"u%d_%d_%d" % (unit, p, v): s for s, (p, v) in enumerate(zip(t["head_pos"].tolist(), t["head_var"].tolist()))}
    off, seq, length = t["seq_off"].tolist(), t["seq"], t["n_nodes"].tolist()
    n = 0
    for line in text.splitlines():
        f = line.split(b"\t")
        assert f[0] == b"P" and f[3] == b"*" and len(f) == 7
        pu, rec, base = (int(x) for x in f[1][1:].split(b"_"))
        segs = [name[s[:-1]] for s in f[2].split(b",")]
        assert pu == unit and all(s.endswith(b"+") for s in f[2].split(b","))
        ln, fs, ls = int(f[4][5:]), int(f[5][5:]), int(f[6][5:])
        assert (f[4][:5], f[5][:5], f[6][:5]) == (b"ln:i:", b"fs:i:", b"ls:i:")
        cat = b"".join(seq[off[s]:off[s + 1]] for s in segs)
        cut = cat[fs:len(cat) - (length[segs[-1]] - 1 - ls)]
        assert len(cut) == ln and cut == recs[rec][base:base + ln], line[:80]
        n += 1
    return n


def check_whole_unit(agx, tmp, unit, k, iv, cov):
    """One unit, whole window at the build's coverage: map, stretches, text, bases.  Returns what the other tests look at."""
    o = H.run_oracle(tmp, unit, k, iv, cov, graph=True)
    g = o["graph"]
    n, ref = g["n_pos"], bytes(g["pos_nuc"])
    wm = WM.build(g, cov)
    with built_unit(agx, tmp, unit, k, iv, cov) as u:
        t = u.unitigs(region=(0, n), min_coverage=cov, id_map=True)
        out = u.finish()
        w = u.walk_paths()
    mu, es, er = PM.id_map(g, cov, 0, n, cov, ref, wm)
    assert same_table(t, mu)
    same_map(t["id_map"], mu["id_map"])
    assert out["pre"] == o["pre"]
    recs = check_stretches(w, out["pre"], wm)
    text = agx.gfa_paths(t, w, unit)
    assert text == PM.paths_gfa(mu, es, er, w, unit)
    assert check_path_bases(text, t, recs, unit) == text.count(b"\n")
    return {"g": g, "wm": wm, "w": w, "t": t, "text": text, "out": out, "o": o}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_walk_units(agx, built, name, tmp_path):
    case = CASES[name]
    iv, cov = getattr(case, "iv", LU.IV), getattr(case, "coverage", 1)
    tmp = WU.write_unit(case.unit, str(tmp_path / "unit"))
    r = check_whole_unit(agx, tmp, 0, LU.K, iv, cov)
    assert len(r["w"]["rec_len"]) > 0 and r["text"].count(b"\n") >= len(r["w"]["rec_len"])      # every record begins on a node of the export


def test_pile_of_variants(agx, built, tmp_path):
    tmp = write_pileup_unit(str(tmp_path / "pile"), 180, spacing=300)
    r = check_whole_unit(agx, tmp, 0, 5, 50, 1)
    m = r["t"]["id_map"]
    assert (m["id_first"] >= m["n_pos"]).sum() >= 179 * 90           # the pile's side ids: a run each (their neighbours in id order are other variants)


@pytest.mark.parametrize("seed", [201, 203])
def test_generated_units(agx, built, seed, tmp_path):
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **next(c for c in CONFIGS if c["seed"] == seed))
    meta = H.read_meta(run)
    joined = breaks = lines = 0
    for unit in range(meta["units"]):
        r = check_whole_unit(agx, os.path.join(run, "tmp"), unit, meta["k"], meta["insert_variation"], meta["coverage"])
        st, j = r["w"]["st_off"].astype(np.int64), r["w"]["joined"]
        inner = np.ones(len(j), bool)
        inner[st[:-1][st[:-1] < len(j)]] = False
        joined += int(j.sum())
        breaks += int((inner & (j == 0)).sum())
        lines += r["text"].count(b"\n")
    assert joined > 0 and lines > 0                      # walks that went on over an edge behind a run's end
    assert (breaks > 0) == (seed == 201)                 # and, on the unit with contigs, walks that came back from a conti-mer chain


def write_piles(run, piles, genome_len=3000, seed=9):
    """A hand-made unit (no contigs): pairs (left, right) of 100-base mates; pairs that share a left-mate alignment add a variant each at its ~96 positions."""
    rnd = random.Random(seed)
    tmp = os.path.join(run, "tmp")
    os.makedirs(tmp, exist_ok=True)
    g = "".join(rnd.choice("ACGT") for _ in range(genome_len))
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    with open(os.path.join(tmp, "_genome.0.fa"), "w") as f:
        f.write(">0\n" + "".join(g[i:i + 60] + "\n" for i in range(0, genome_len, 60)))
    open(os.path.join(tmp, "_contigs.fa"), "w").close()
    open(os.path.join(tmp, "_contigs_genome.0.psl"), "w").close()
    with open(os.path.join(tmp, "_reads.fa"), "w") as rf, open(os.path.join(tmp, "_reads_genome.0.bowtie"), "w") as sf:
        for i, (left, right) in enumerate(piles):
            m1 = g[left:left + 100]
            m2 = "".join(comp[c] for c in reversed(g[right:right + 100]))
            rf.write(">%d\n%s\n>%d\n%s\n" % (i, m1, i, m2))
            sf.write("%d\t99\t0\t%d\t42\t100M\t=\t%d\t%d\t*\t*\n" % (i, left + 1, right + 1, right + 100 - left))
            sf.write("%d\t147\t0\t%d\t42\t100M\t=\t%d\t%d\t*\t*\n" % (i, right + 1, left + 1, -(right + 100 - left)))
    return tmp


def test_window_edges(agx, built, tmp_path):
    """Two variants at positions 0 .. 95 (one side id per position: consecutive side ids are consecutive nodes of one unitig), one at 100 .. 195, three at 200 .. 295, single ones further on: side ids
    on both sides of every cut; windows from every pair of cuts."""
    piles = [(0, 1000), (0, 1400), (100, 2000), (200, 1100), (200, 1500), (200, 1950), (600, 2900), (1000, 2900), (1400, 2900), (2500, 2900)]
    tmp = write_piles(str(tmp_path / "piles"), piles)
    o = H.run_oracle(tmp, 0, 5, 50, 1, graph=True)
    g = o["graph"]
    n, ref = g["n_pos"], bytes(g["pos_nuc"])
    wm = WM.build(g, 1)
    sx = wm["side_xpos"].astype(np.int64)
    cuts = [0, 1, 63, 64, 65, 127, 128, 255, 256, 257, n - 1, n]
    assert cuts == sorted(cuts)
    for c in cuts[1:-2]:
        assert (sx < c).any() and (sx >= c).any()
    seen = set()
    with built_unit(agx, tmp, 0, 5, 50, 1) as u:
        maps = {}
        for lo in cuts:
            for hi in cuts:
                if lo > hi:
                    continue
                t = u.unitigs(region=(lo, hi), min_coverage=1, id_map=True)
                mu, es, er = PM.id_map(g, 1, lo, hi, 1, ref, wm)
                assert same_table(t, mu), (lo, hi)
                same_map(t["id_map"], mu["id_map"])
                maps[(lo, hi)] = (t, mu, es, er)
                m = mu["id_map"]
                sides = int(((sx >= lo) & (sx < hi)).sum())
                main, side = m["id_first"] < n, m["id_first"] >= n
                if lo == hi:
                    seen.add("empty")
                    assert len(m["id_first"]) == 0 and len(t["head_pos"]) == 0
                elif sides == 0 and len(m["id_first"]):
                    seen.add("no side id")
                # window ids: main id a is lo + i, the window's j-th side id is (hi - lo) + j
                wf = np.where(main, m["id_first"].astype(np.int64) - lo, (hi - lo) + m["id_first"].astype(np.int64) - n - int((sx < lo).sum()))
                wl = wf + (m["id_last"].astype(np.int64) - m["id_first"].astype(np.int64))
                for edge in (64, 256):
                    if ((wf < edge) & (wl >= edge)).any():
                        seen.add("run across %d" % edge)
                    if ((wf < edge) & (wl >= edge) & side).any():
                        seen.add("side run across %d" % edge)
                if main.any() and side.any() and m["id_last"][main].max() == hi - 1 and m["id_first"][side].min() == n + int((sx < lo).sum()):
                    seen.add("last main id next to the first side id")
        assert len(maps) == 78
        out = u.finish()
        w = u.walk_paths()
    assert out["pre"] == o["pre"]
    assert seen >= {"empty", "no side id", "run across 64", "run across 256", "side run across 64", "last main id next to the first side id"}, seen
    recs = check_stretches(w, out["pre"], wm)
    for (lo, hi), (t, mu, es, er) in maps.items():
        text = agx.gfa_paths(t, w, 0)
        assert text == PM.paths_gfa(mu, es, er, w, 0), (lo, hi)
        check_path_bases(text, t, recs, 0)


def test_thresholds(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), sam_seq=0, **next(c for c in CONFIGS if c["seed"] == 201))      # 60 kb with contigs, built at coverage 5
    meta = H.read_meta(run)
    tmp = os.path.join(run, "tmp")
    k, iv, c = meta["k"], meta["insert_variation"], meta["coverage"]
    o = H.run_oracle(tmp, 0, k, iv, c, graph=True)
    g = o["graph"]
    n, ref = g["n_pos"], bytes(g["pos_nuc"])
    wm = WM.build(g, c)
    key, cnt = g["node_key"].reshape(-1, 6), g["node_cnt"].reshape(-1, 6)
    reads_only = key[:, 0] == M.NONE
    assert reads_only.any() and (~reads_only).any()
    above = int(cnt[reads_only, 0].max()) + 1            # one above every read-only node's coverage: only contig nodes survive
    got = {}
    with built_unit(agx, tmp, 0, k, iv, c) as u:
        for cov in (0, c, above):
            t = u.unitigs(min_coverage=cov, id_map=True)
            mu, es, er = PM.id_map(g, c, 0, n, cov, ref, wm)
            assert same_table(t, mu), cov
            same_map(t["id_map"], mu["id_map"])
            got[cov] = (t, mu, es, er)
        out = u.finish()
        w = u.walk_paths()
    recs = check_stretches(w, out["pre"], wm)
    text = {}
    for cov, (t, mu, es, er) in got.items():
        text[cov] = agx.gfa_paths(t, w, 0)
        assert text[cov] == PM.paths_gfa(mu, es, er, w, 0), cov
        check_path_bases(text[cov], t, recs, 0)
    mapped = {cov: int((got[cov][0]["id_map"]["id_last"].astype(np.int64) - got[cov][0]["id_map"]["id_first"] + 1).sum()) for cov in got}
    assert mapped[0] == mapped[c] == int(wm["has"].sum())                 # at 0 (and at the build's coverage) every walk node is mapped ...
    assert got[0][0]["n_nodes"].mean() < got[c][0]["n_nodes"].mean()      # ... and at 0 the segments are shorter: the pruned nodes are back, with their branches
    assert text[0] != text[c]
    assert mapped[above] < mapped[c] and text[above].count(b"\n") != text[c].count(b"\n")      # above, paths break at the dead nodes (where: the model's text)


def test_walkers_download_forms_and_unit_kinds_give_the_same(agx, built, tmp_path, monkeypatch):
    run = H.synth(str(tmp_path / "run"), seed=79, chroms="150000", pairs=30000, coverage=4, read_indel=0.2, multi=0.2, contig_overlap=0.3, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    o = H.run_oracle(tmp, 0, 5, 50, 4, graph=True)
    g = o["graph"]
    n, ref = g["n_pos"], bytes(g["pos_nuc"])
    wm = WM.build(g, 4)
    mu, es, er = PM.id_map(g, 4, 0, n, 4, ref, wm)

    def one(flags=0, trim=False):
        with built_unit(agx, tmp, 0, 5, 50, 4, flags=flags) as u:
            t = u.unitigs(min_coverage=4, id_map=True)
            if trim:
                u.download()
                u.trim()
            out = u.finish()
            w = u.walk_paths()
        assert out["pre"] == o["pre"]
        return w, agx.gfa_paths(t, w, 0)

    w0, text0 = one()                                    # one walker (a unit this small is not split), the download streamed or not as the engine decides
    check_stretches(w0, o["pre"], wm)
    assert text0 == PM.paths_gfa(mu, es, er, w0, 0) and text0.count(b"\n") > 100
    monkeypatch.setenv("AGX_WALK_SPLIT_MIN", "0")
    monkeypatch.setenv("AGX_WALK_POISON", "1")
    monkeypatch.setenv("AGX_WALK_SPLIT_WARMUP", "20000")
    modes = 0
    for walkers in ("2", "16"):
        monkeypatch.setenv("AGX_WALK_SPLIT_WALKERS", walkers)
        for env in ({"AGX_STREAM_PIECES": "2"}, {"AGX_STREAM_PIECES": "16"}, {"AGX_NO_STREAM_DOWNLOAD": "1"}):
            for k2, v2 in env.items():
                monkeypatch.setenv(k2, v2)
            for flags, trim in ((0, False), (agx.AGX_FLAG_ONE_SHOT, False), (0, True)):
                w, text = one(flags, trim)
                assert same_stretches(w, w0) and text == text0, (walkers, env, flags, trim)
                modes += 1
            for k2 in env:
                monkeypatch.delenv(k2)
    assert modes == 18


def test_disturbs_nothing(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), seed=211, chroms="60000", pairs=20000, coverage=5, contig_min=1500, contig_max=3000, sam_seq=0)
    tmp = os.path.join(run, "tmp")
    with built_unit(agx, tmp, 0, 5, 50, 5, keep_paths=False) as u:
        n = u.stats()["n_pos"]
        whole, table, win = u.gfa(0), u.unitigs(), u.unitigs(region=(100, 5000), min_coverage=1)
        fin = u.finish()
        planned = u.hbm_needed()
    with built_unit(agx, tmp, 0, 5, 50, 5) as u:
        assert u.hbm_needed() >= planned                # the id map's scratch is part of the unit's block (whole blocks: a small unit's may round to the same number), so no export asks the device for memory: device_bytes below
        before = u.stats()["device_bytes"]
        a = u.unitigs(region=(100, 5000), min_coverage=1, id_map=True)              # mapped first, on scratch no export has touched
        assert u.gfa(0) == whole and same_table(u.unitigs(), table)
        b = u.unitigs(region=(100, 5000), min_coverage=1, id_map=True)              # mapped after the whole export
        assert same_table(u.unitigs(region=(100, 5000), min_coverage=1), win)
        c = u.unitigs(region=(0, n), min_coverage=0, id_map=True)
        d = u.unitigs(region=(100, 5000), min_coverage=1, id_map=True)              # after a larger map
        assert same_table(a, win) and same_table(b, win) and same_table(d, win) and same_table(c, u.unitigs(min_coverage=0))
        for x in (b, d):
            same_map(x["id_map"], a["id_map"])
        assert u.gfa(0) == whole
        assert u.stats()["device_bytes"] == before
        assert u.finish() == fin
        assert u.finish() == fin                         # and again: the stretches are those of the last finish
        w = u.walk_paths()
        assert len(w["rec_len"]) == fin["pre"].count(b">")
    with built_unit(agx, tmp, 0, 5, 50, 5, keep_paths=False) as u:      # without the flag a unit plans the bytes it planned
        assert u.hbm_needed() == planned


def test_refusals(agx, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), seed=212, chroms="30000", pairs=8000, coverage=5, sam_seq=0)
    tmp = os.path.join(run, "tmp")

    def refused(f, *a, **kw):
        with pytest.raises(agx.AgxError) as e:
            f(*a, **kw)
        assert e.value.code == agx.AGX_E_ARG
        return e.value.msg

    with built_unit(agx, tmp, 0, 5, 50, 5, keep_paths=False) as u:
        assert "KEEP_PATHS" in refused(u.unitigs, region=(0, 10), id_map=True)
        u.finish()
        assert "KEEP_PATHS" in refused(u.walk_paths)
    with built_unit(agx, tmp, 0, 5, 50, 5, keep_counts=False) as u:
        assert "KEEP_COUNTS" in refused(u.unitigs, region=(0, 10), id_map=True)
        u.finish()
        assert len(u.walk_paths()["rec_len"]) > 0       # the stretches need no counts
    with built_unit(agx, tmp, 0, 5, 50, 5) as u:
        n = u.stats()["n_pos"]
        refused(u.walk_paths)                            # before a finish
        assert "[10, 9)" in refused(u.unitigs, region=(10, 9), id_map=True)
        refused(u.unitigs, region=(0, n + 1), id_map=True)
        assert len(u.unitigs(region=(n, n), id_map=True)["id_map"]["id_first"]) == 0
        u.finish()
        w = u.walk_paths()
        u.download()
        u.trim()
        refused(u.unitigs, region=(0, 10), id_map=True)  # after trim
        assert same_stretches(u.walk_paths(), w)         # (the stretches outlive the trim)
        u.release()
        refused(u.walk_paths)
    with built_unit(agx, tmp, 0, 5, 50, 5, flags=agx.AGX_FLAG_ONE_SHOT) as u:
        u.download()
        refused(u.unitigs, region=(0, 10), id_map=True)  # a one-shot unit after its download
        u.finish()
        assert same_stretches(u.walk_paths(), w)
