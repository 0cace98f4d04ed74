"""AlignGraph_amd --graphBubbles <file> [--graphBubblesMax n]: the file is, unit by unit, the bubbles model's text (tests/bubbles_model.py on the region model's table of
the oracle's graph) — with --graphRegion of that unit's window alone, with --graphMinCoverage at that threshold, with --graphEdgeSupport the library's text with the
branches' support —; the per-unit files in tmp/ carry the settings in their names; a --resume that redoes the last unit gives the same file; the option works without
--graphOut and beside it; everything the reference writes stays byte for byte as it is, and without the option the run writes what it wrote before the option existed."""
import os

import pytest

import bubbles_model as BM
import harness as H
import unitig_region_model as R
from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)
from test_cli_graph import option
from test_cli_graph_region import usage_shown


def settings(c):
    return option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)


def model_texts(c, units, region=None, min_cov=None, max_nodes=None):
    """The expected per-unit TSV texts."""
    k, iv, cov = settings(c)
    out = []
    for unit in units:
        g = H.run_oracle(os.path.join(c.work, "tmp"), unit, k, iv, cov, graph=True)["graph"]
        lo, hi = region if region else (0, int(g["n_pos"]))
        t = R.region_unitigs(g, lo, hi, cov if min_cov is None else min_cov, bytes(g["pos_nuc"]))
        out.append(BM.tsv(BM.bubbles(t, None, max_nodes), unit))
    return out


def unchanged(c, p, extra):
    assert p.returncode == 0, p.stdout[-400:]
    assert strip_time(p.stdout) == strip_time(c.expected("stdout.txt"))
    for fn in FINALS:
        if os.path.exists(os.path.join(c.exp, fn)):
            assert c.got(fn) == c.expected(fn), fn
    for fn in os.listdir(os.path.join(c.exp, "tmp")):
        if fn == "_command.txt":
            assert c.got("tmp/" + fn) == c.expected("tmp/" + fn) + "".join(a + "\n" for a in extra).encode()
        else:
            assert c.got("tmp/" + fn) == c.expected("tmp/" + fn), fn


def parts_of(c):
    return sorted(f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_bubbles."))


@pytest.mark.gpu
def test_the_option_alone_and_resume(cli, built, tmp_path):
    c = Case("default", tmp_path)
    extra = ["--graphBubbles", "sites.tsv"]
    unchanged(c, c.run(cli, [a for a in c.args if a] + extra), extra)
    texts = model_texts(c, range(c.units))
    parts = ["_bubbles.%d.tsv" % u for u in range(c.units)]
    assert parts_of(c) == sorted(parts)
    for fn, text in zip(parts, texts):
        assert c.got("tmp/" + fn) == text, fn
    got = c.got("sites.tsv")
    assert got == b"".join(texts) and got
    assert all(line.count(b"\t") == 10 and line.startswith(b"u") and line.split(b"\t")[8:10] == [b".", b"."] for line in got.splitlines())
    assert not [f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_graph.")], "no graph output was asked for"
    # --resume that redoes the last unit: its outputs and its part removed, the checkpoint rewound
    last = c.units - 1
    for stem in ("_initial_contigs", "_pre_extended_contigs", "_extended_contigs"):
        os.remove(os.path.join(c.work, "tmp", "%s.%d.fa" % (stem, last)))
    os.remove(os.path.join(c.work, "tmp", parts[last]))
    os.remove(os.path.join(c.work, "sites.tsv"))
    with open(os.path.join(c.work, "tmp", "_checkpoint.txt"), "w") as f:
        f.write("0\n%d\n" % last)
    p = c.run(cli, ["--resume"])
    assert p.returncode == 0 and b"RESUMED SUCCESSFULLY :-)" in p.stdout
    assert c.got("sites.tsv") == b"".join(texts) and c.got("tmp/" + parts[last]) == texts[last]
    for fn in ("e.fa", "r.fa"):
        assert c.got(fn) == c.expected(fn), fn


@pytest.mark.gpu
def test_with_graph_out_threshold_and_max(cli, built, tmp_path):
    """Beside --graphOut, at --graphMinCoverage 0 and with branches of one node at most: the GFA is what the run writes without --graphBubbles."""
    c, plain = Case("default", tmp_path / "with"), Case("default", tmp_path / "without")
    graph = ["--graphOut", "g.gfa", "--graphMinCoverage", "0"]
    extra = graph + ["--graphBubbles", "sites.tsv", "--graphBubblesMax", "1"]
    unchanged(c, c.run(cli, [a for a in c.args if a] + extra), extra)
    assert plain.run(cli, [a for a in plain.args if a] + graph).returncode == 0
    assert c.got("g.gfa") == plain.got("g.gfa") and c.got("g.gfa").count(b"\nL\t") > 0
    texts = model_texts(c, range(c.units), min_cov=0, max_nodes=1)
    assert c.got("sites.tsv") == b"".join(texts)
    assert parts_of(c) == sorted("_bubbles.%d.c0.m1.tsv" % u for u in range(c.units))
    every = b"".join(model_texts(c, range(c.units), min_cov=0))
    assert set(c.got("sites.tsv").splitlines()) <= set(every.splitlines())


@pytest.mark.gpu
def test_with_a_region_and_with_support(cli, built, tmp_path):
    import aligngraph_amd as A
    c = Case("default", tmp_path / "region")
    extra = ["--graphRegion", "0:100-900", "--graphBubbles", "sites.tsv", "--graphMinCoverage", "1"]
    unchanged(c, c.run(cli, [a for a in c.args if a] + extra), extra)
    assert c.got("sites.tsv") == model_texts(c, [0], region=(100, 900), min_cov=1)[0]
    assert parts_of(c) == ["_bubbles.0.100-900.c1.tsv"]
    s = Case("default", tmp_path / "support")
    extra = ["--graphBubbles", "sites.tsv", "--graphEdgeSupport", "--graphMinCoverage", "1"]
    unchanged(s, s.run(cli, [a for a in s.args if a] + extra), extra)
    k, iv, cov = settings(s)
    want = b""
    for unit in range(s.units):
        with A.Unit(k=k, insert_variation=iv, coverage=cov, keep_counts=True, edge_support=True) as e:
            e.load_files(os.path.join(s.work, "tmp"), unit)
            e.upload()
            e.build()
            t = e.unitigs(min_coverage=1, edge_support=True)
            want += BM.tsv(BM.bubbles(t, t["link_support"]), unit)
    assert s.got("sites.tsv") == want and parts_of(s) == sorted("_bubbles.%d.c1.s.tsv" % u for u in range(s.units))
    plain = b"".join(model_texts(s, range(s.units), min_cov=1))
    assert [l.split(b"\t")[:8] for l in want.splitlines()] == [l.split(b"\t")[:8] for l in plain.splitlines()] and b"\t.\t." not in want


@pytest.mark.gpu
def test_without_the_option_nothing_new_is_written(cli, tmp_path):
    c = Case("default", tmp_path)
    unchanged(c, c.run(cli, [a for a in c.args if a]), [])
    assert not parts_of(c) and not [f for f in os.listdir(c.work) if f.endswith(".tsv")]


def test_option_syntax(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    for bad in (["--graphBubbles"], ["--graphBubblesMax", "2"], ["--graphBubbles", "b.tsv", "--graphBubblesMax", "-1"], ["--graphBubbles", "b.tsv", "--graphBubblesMax", "two"],
                ["--graphBubbles", "b.tsv", "--graphBubbles", "c.tsv"], ["--graphBubbles", "b.tsv", "--graphPaths"], ["--graphMinCoverage", "3"], ["--graphEdgeSupport"],
                ["--graphRegion", "0:100-900"]):
        p = c.run(cli, args + bad)
        assert usage_shown(p) and b"graphBubbles" not in p.stdout, bad      # the reference's usage text does not name the option


def test_option_is_accepted(cli, tmp_path):
    """Past the parser the run goes on as any other: without a device up to the loud stop in front of the unit loop.  Region, threshold and support are accepted without
    --graphOut."""
    import aligngraph_amd as A
    c = Case("default", tmp_path)
    extra = ["--graphRegion", "0:100-900", "--graphMinCoverage", "2", "--graphEdgeSupport", "--graphBubbles", "b.tsv", "--graphBubblesMax", "4"]
    p = c.run(cli, [a for a in c.args if a] + extra)
    assert b"(0) Alignment finished" in p.stdout and not usage_shown(p)
    if A.device_count() > 0:
        assert p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout
        assert os.path.exists(os.path.join(c.work, "tmp", "_bubbles.0.100-900.c2.s.m4.tsv"))
    else:
        assert p.returncode == 255 and b"NO HIP DEVICE" in p.stdout
    assert c.got("tmp/_command.txt").endswith(("".join(a + "\n" for a in extra)).encode())
