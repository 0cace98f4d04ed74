"""AlignGraph_amd --graphEdgeReads <file> [--graphEdgeReadsMax n]: the file is, unit by unit, the TSV text of Unit.edge_reads() at that threshold (default 2) — with
--graphRegion of that unit's window alone —, the per-unit files carry threshold and region in their names, and a run with the option writes the same contig files and
prints the same lines as one without it, which in turn are the expected ones."""
import os
import re

import pytest

from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)
from test_cli_graph import option
from test_cli_graph_region import usage_shown


def units_of(c):
    return sorted(int(m.group(1)) for m in (re.fullmatch(r"_genome\.(\d+)\.fa", f) for f in os.listdir(os.path.join(c.work, "tmp"))) if m)


def library_text(c, units, region, top):
    """What the library gives for the run's units: Unit.edge_reads() as TSV, unit after unit"""
    import aligngraph_amd as A
    k, iv, cov = option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)
    out = b""
    for u in units:
        with A.Unit(k=k, insert_variation=iv, coverage=cov, keep_counts=True, edge_support=True) as e:
            e.load_files(os.path.join(c.work, "tmp"), u)
            e.upload()
            e.build()
            out += A.edge_reads_tsv(e.edge_reads(region, top), u)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("extra,region,top", [([], None, 2), (["--graphEdgeReadsMax", "1"], None, 1), (["--graphRegion", "0:100-900", "--graphEdgeReadsMax", "3"], (100, 900), 3)],
                         ids=["default", "max1", "region"])
def test_graph_edge_reads(cli, built, extra, region, top, tmp_path):
    c = Case("default", tmp_path / "with")
    plain = Case("default", tmp_path / "without")
    base = [a for a in c.args if a]
    p = c.run(cli, base + ["--graphEdgeReads", "reads.tsv"] + extra)
    q = plain.run(cli, base)
    assert p.returncode == 0 and q.returncode == 0, p.stdout[-400:]
    assert strip_time(p.stdout) == strip_time(q.stdout) == strip_time(c.expected("stdout.txt"))
    for fn in FINALS:      # the outputs of both runs are the expected bytes
        if os.path.exists(os.path.join(c.exp, fn)):
            assert c.got(fn) == plain.got(fn) == c.expected(fn), fn
    units = units_of(c)
    got = c.got("reads.tsv")
    assert got == library_text(c, [0] if region else units, region, top)
    lines = got.split(b"\n")[:-1]
    assert lines and all(len(ln.split(b"\t")) == 7 and 1 <= int(ln.split(b"\t")[5]) <= top and ln.split(b"\t")[6].count(b",") + 1 == int(ln.split(b"\t")[5]) for ln in lines)
    # the per-unit files carry the threshold and the region in their names; a run without the option writes none
    parts = sorted(f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_edge_reads."))
    assert parts == ["_edge_reads.%d%s.m%d.tsv" % (u, ".100-900" if region else "", top) for u in ([0] if region else units)]
    assert not [f for f in os.listdir(os.path.join(plain.work, "tmp")) if f.startswith("_edge_reads.")] and not os.path.exists(os.path.join(plain.work, "reads.tsv"))
    assert b"--graphEdgeReads\nreads.tsv\n" in c.got("tmp/_command.txt")


def test_option_syntax(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    assert usage_shown(c.run(cli, args + ["--graphEdgeReads"]))                                               # no file
    assert usage_shown(c.run(cli, args + ["--graphEdgeReadsMax", "2"]))                                       # the threshold alone
    assert usage_shown(c.run(cli, args + ["--graphEdgeReads", "r.tsv", "--graphEdgeReadsMax", "-1"]))
    assert usage_shown(c.run(cli, args + ["--graphEdgeReads", "r.tsv", "--graphEdgeReadsMax", "two"]))
    assert usage_shown(c.run(cli, args + ["--graphEdgeReads", "r.tsv", "--graphEdgeReads", "s.tsv"]))         # a second time
    assert usage_shown(c.run(cli, args + ["--graphRegion", "0:100-900"]))                                     # a region still needs one of the two outputs it cuts
    p = c.run(cli, args + ["--graphEdgeReads"])
    assert b"graphEdgeReads" not in p.stdout      # the reference's usage text does not name the option


def test_option_is_accepted(cli, tmp_path):
    """Past the parser the run goes on as any other: without a device up to the loud stop in front of the unit loop.  A region without --graphOut is accepted with it."""
    import aligngraph_amd as A
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a] + ["--graphRegion", "0:100-900", "--graphEdgeReads", "r.tsv", "--graphEdgeReadsMax", "4"])
    assert b"(0) Alignment finished" in p.stdout and not usage_shown(p)
    if A.device_count() > 0:
        assert p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout
    else:
        assert p.returncode == 255 and b"NO HIP DEVICE" in p.stdout
    assert c.got("tmp/_command.txt").endswith(b"--graphEdgeReads\nr.tsv\n--graphEdgeReadsMax\n4\n")
