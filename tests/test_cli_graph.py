"""AlignGraph_amd --graphOut: the end-to-end cases of test_cli.py with the option appended.  Everything the reference writes stays byte for
byte as it is, and g.gfa is the GFA header followed by the unitig model's text of every unit (tests/unitig_model.py on the oracle's graph), also
after a --resume that has to redo the last unit."""
import os

import pytest

import harness as H
import unitig_model as M
from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)

def option(args, name, default):
    return int(args[args.index(name) + 1]) if name in args else default


def model_gfa(c):
    k, iv, cov = option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)
    tmp = os.path.join(c.work, "tmp")
    out = [M.GFA_HEADER]
    for u in range(c.units):
        o = H.run_oracle(tmp, u, k, iv, cov, graph=True)
        out.append(M.unit_gfa(o["graph"], cov, M.read_reference(tmp, u), u))
    return b"".join(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "flags"])
def test_graph_out(cli, built, name, tmp_path):
    c = Case(name, tmp_path)
    args = [a for a in c.args if a] + ["--graphOut", "g.gfa"]
    p = c.run(cli, args)
    assert p.returncode == 0, p.stdout[-400:]
    assert strip_time(p.stdout) == strip_time(c.expected("stdout.txt"))
    for fn in FINALS:
        if os.path.exists(os.path.join(c.exp, fn)):
            assert c.got(fn) == c.expected(fn), fn
    for fn in os.listdir(os.path.join(c.exp, "tmp")):
        if fn == "_command.txt":            # the command line itself, with the option
            assert c.got("tmp/" + fn) == c.expected("tmp/" + fn) + b"--graphOut\ng.gfa\n"
        else:
            assert c.got("tmp/" + fn) == c.expected("tmp/" + fn), fn
    want = model_gfa(c)
    assert want.count(b"\nS\t") > 0
    assert c.got("g.gfa") == want
    # --resume that redoes the last unit: its outputs and its graph file removed, the checkpoint rewound
    last = c.units - 1
    for stem in ("_initial_contigs", "_pre_extended_contigs", "_extended_contigs"):
        os.remove(os.path.join(c.work, "tmp", "%s.%d.fa" % (stem, last)))
    os.remove(os.path.join(c.work, "tmp", "_graph.%d.gfa" % last))
    os.remove(os.path.join(c.work, "g.gfa"))
    with open(os.path.join(c.work, "tmp", "_checkpoint.txt"), "w") as f:
        f.write("0\n%d\n" % last)
    p = c.run(cli, ["--resume"])
    assert p.returncode == 0 and b"RESUMED SUCCESSFULLY :-)" in p.stdout
    for fn in ("e.fa", "r.fa"):
        assert c.got(fn) == c.expected(fn), fn
    assert c.got("g.gfa") == want


def test_graph_out_is_checked_at_parse_time(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    p = c.run(cli, args + ["--graphOut", "no/such/dir/g.gfa"])
    assert b"CANNOT OPEN FILE!" in p.stdout
    p = c.run(cli, args + ["--graphOut", "g.gfa", "--graphOut", "h.gfa"])      # a second time: usage, as for every other option
    assert b"AlignGraph --read1" in p.stdout and p.returncode != 0
