"""The two binary doors into the engine refuse damaged content (CPU): tests/damaged_inputs.py is the table, this is what holds the checks to it.

  * every entry of the table gives its stated verdict — `accepted`, or the name of the rule that refuses it — on the checks the loaders run (agx_load.cpp "content rules",
    through the serial executor's library);
  * every rule name the checks can return is the verdict of some entry: a rule cannot arrive without a damaged input that it refuses;
  * nothing the loaders really write is refused: every unit of tests/test_staged_pairs.py's settings and every golden fixture unit passes both checks;
  * what the checks let through stays inside its buffers: tests/damaged_inputs_san.cpp, a stand-alone program under the host sanitizers, runs a seeded list of
    single-field mutants through the checks and the accepted ones through everything that reads those arrays before and during a build.
Nothing here needs or touches a device."""
import ctypes
import json
import os
import subprocess

import pytest

import harness as H
import damaged_inputs as D
from hostsim import sim
from test_staged_pairs import SETTINGS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# the small unit with every structure present: indels, clips, multi-hits, both left-mate choices, bases that are not A, C, G, T
SMALL = dict(seed=21, chroms="8000", pairs=1500, coverage=5, read_indel=0.3, read_clip=0.2, read_badclip=0.05, multi=0.5, multi_near=0.4, read_n=0.01, mate1_left=0.3, sam_seq=0, threads=2, pairs_bin=2)
K, BATCH = 5, 1000000


@pytest.fixture(scope="module")
def small(built, tmp_path_factory):
    run = H.synth(str(tmp_path_factory.mktemp("damaged") / "run"), **SMALL)
    return os.path.join(run, "tmp")


@pytest.fixture(scope="module")
def doors(small, tmp_path_factory):
    scratch = str(tmp_path_factory.mktemp("damaged_files"))
    cache = D.CacheDoor(small, 0, K, BATCH)
    d = {"cache": cache, "cache_fast": D.CacheDoor(small, 0, K, BATCH, fast=True), "cache_header": D.CacheDoor(small, 0, K, BATCH, header=True),
         "pairs": D.PairsDoor(os.path.join(small, "_agx_pairs.0.bin"), cache.n["n_pos"], scratch, K, BATCH)}
    yield d
    for k in ("cache", "cache_fast", "cache_header"):
        d[k].close()


def test_the_small_unit_has_every_structure(doors):
    for d in (doors["pairs"], doors["cache"]):
        h = d.a["hits"]
        assert d.n["n_sides"] > 50 and d.n["n_runs"] > 100 and d.n["n_jump"] > 20 and d.n["n_other"] > 10 and (h["back"] != 0).sum() > 10
        assert (h["flags"] & D.LEFT2).any() and not (h["flags"] & D.LEFT2).all() and (h["flags"] & D.REV1).any() and (h["flags"] & D.REV2).any()
        assert d.verdict() == D.ACCEPTED
    assert doors["cache"].n["n_segs"] > 2 and doors["cache"].n["n_chain_end"] > 0
    assert doors["cache_fast"].verdict() == D.ACCEPTED and doors["cache_header"].verdict() == D.ACCEPTED
    assert doors["pairs"].a["hits"].tobytes() == doors["cache"].a["hits"].tobytes()      # (the same staged arrays behind both doors)


@pytest.mark.parametrize("name,door", [(e.name, k) for e in D.TABLE for k in e.doors])
def test_entry_gives_its_verdict(doors, name, door):
    e, d = D.BY_NAME[name], doors[door]
    d.restore()
    try:
        e.apply(d)
        got = d.verdict()
    finally:
        d.restore()
    assert got == e.verdict, "%s on %s: %s, the table says %s" % (name, door, got, e.verdict)
    assert d.verdict() == D.ACCEPTED      # (restored)


def test_every_rule_has_an_entry_that_it_refuses():
    names = set(D.rule_names())
    refused = {e.verdict for e in D.TABLE if e.verdict != D.ACCEPTED}
    assert refused <= names, "the table names rules the checks do not have: %s" % sorted(refused - names)
    assert names <= refused, "rules without a refused entry in tests/damaged_inputs.py: %s" % sorted(names - refused)


def _both_checks(tmp, unit, k, batch, scratch):
    """A unit as the loaders write it passes the cache's checks (both loaders) and the pairs file's."""
    for fast in (False, True):
        try:
            c = D.CacheDoor(tmp, unit, k, batch, fast=fast)
        except sim.SimError as e:
            assert fast and "declined" in e.msg, e.msg      # (the fast loader may decline a unit: the general one serves it)
            continue
        n_pos = c.n["n_pos"]
        assert c.verdict() == D.ACCEPTED, (tmp, unit, fast, c.verdict())
        c.header = True
        assert c.verdict() == D.ACCEPTED, (tmp, unit, fast, "header", c.verdict())
        c.close()
    path = os.path.join(tmp, "_agx_pairs.%d.bin" % unit)
    if not os.path.exists(path):      # (a unit that exists as text only: the file the text stages to)
        path = os.path.join(scratch, "_agx_pairs.%d.bin" % unit)
        msg = ctypes.create_string_buffer(512)
        L = D._lib()
        L.agx_hostsim_write_pairs_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        assert L.agx_hostsim_write_pairs_file(tmp.encode(), unit, k, batch, 2, path.encode(), msg, 512) == 0, msg.value
    p = D.PairsDoor(path, n_pos, scratch, k, batch)
    assert p.verdict() == D.ACCEPTED, (tmp, unit, p.verdict())


@pytest.mark.parametrize("cfg", SETTINGS, ids=lambda c: "seed%d" % c["seed"])
def test_no_false_refusals_settings(cfg, built, tmp_path):
    run = H.synth(str(tmp_path / "run"), sam_seq=0, threads=3, pairs_bin=2, **cfg)
    meta = H.read_meta(run)
    for u in range(meta["units"]):
        _both_checks(os.path.join(run, "tmp"), u, meta["k"], BATCH, str(tmp_path))


@pytest.mark.parametrize("batch", [7, 1000, 1999, 2000, 2001, 6000])
def test_no_false_refusals_batch_sizes(built, tmp_path, batch):
    run = H.synth(str(tmp_path / "run"), seed=11, chroms="30000,20000", pairs=6000, coverage=5, multi=0.6, multi_near=0.3, read_indel=0.3, read_clip=0.2, sam_seq=0, threads=2, pairs_bin=2, batch=batch)
    for u in range(2):
        _both_checks(os.path.join(run, "tmp"), u, 5, batch, str(tmp_path))


def test_no_false_refusals_placeholder_reads(built, tmp_path):
    kw = dict(chroms="40000,30000,20000", pairs=9000, coverage=4, read_indel=0.2, multi=0.3, sam_seq=0, threads=3, batch=2000)
    a = H.synth(str(tmp_path / "a"), seed=9, pairs_bin=2, oracle_units="0,2", **kw)
    b = H.synth(str(tmp_path / "b"), seed=13, pairs_bin=1, lean=1, oracle_units="1", **kw)
    for run, units in ((a, (0, 2)), (b, (1,))):
        for u in units:
            _both_checks(os.path.join(run, "oracle_%d" % u, "tmp"), u, 5, 2000, str(tmp_path))


def test_no_false_refusals_golden(golden, built, tmp_path):
    units = golden.params.get("units", 1)
    for u in range(units):
        _both_checks(golden.tmp, u, golden.params["k"], BATCH, str(tmp_path))


SAN_MUTANTS, SAN_SEED = 600, 1      # (profiles/damaged_inputs.txt: the length and the time)


def test_what_the_checks_accept_stays_inside_its_buffers(small, tmp_path):
    """tests/damaged_inputs_san.cpp under the host sanitizers: a report ends it non-zero.  The intact unit is accepted and runs clean; mutants fall on both sides."""
    exe = str(tmp_path / "damaged_inputs_san")
    csrc = os.path.join(ROOT, "aligngraph_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-o", exe, os.path.join(HERE, "damaged_inputs_san.cpp")] +
                          [os.path.join(csrc, f) for f in ("agx_host.cpp", "agx_walk.cpp", "agx_load.cpp")])
    r = subprocess.run([exe, small, "0", str(K), str(SAN_MUTANTS), str(SAN_SEED)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "intact: accepted, clean"
    t = lines[-1].replace(":", "").replace(",", "").split()      # mutants N: refused R, accepted and clean C, accepted and refused later L
    n, refused, clean, later = int(t[1]), int(t[3]), int(t[7]), int(t[12])
    assert n == SAN_MUTANTS and refused > 0 and clean > 0 and refused + clean + later <= n
    named = {ln.split()[1].rstrip(":") for ln in lines if ln.startswith("refused ")}
    assert named <= set(D.rule_names())
