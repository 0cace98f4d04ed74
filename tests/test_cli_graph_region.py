"""AlignGraph_amd --graphOut with --graphRegion <unit>:<lo>-<hi> and --graphMinCoverage <n>: the end-to-end cases of test_cli_graph.py with a window.
Everything the reference writes stays byte for byte as it is; g.gfa is the GFA header followed by the region model's lines of the named unit
(tests/unitig_region_model.py on the oracle's graph); the per-unit files in tmp/ carry the settings in their names, so a --resume run under other
settings never merges lines made under these.  Without --graphOut, or malformed, the options print usage like every other malformed option."""
import os

import pytest

import harness as H
import unitig_model as M
import unitig_region_model as R
from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)
from test_cli_graph import option


def model_region_gfa(c, unit, lo, hi, min_cov):
    k, iv, cov = option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)
    tmp = os.path.join(c.work, "tmp")
    o = H.run_oracle(tmp, unit, k, iv, cov, graph=True)
    return M.GFA_HEADER + R.region_gfa(o["graph"], lo, hi, min_cov, M.read_reference(tmp, unit), unit)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "flags"])
def test_graph_region(cli, built, name, tmp_path):
    c = Case(name, tmp_path)
    extra = ["--graphOut", "g.gfa", "--graphRegion", "0:100-900", "--graphMinCoverage", "1"]
    p = c.run(cli, [a for a in c.args if a] + extra)
    assert p.returncode == 0, p.stdout[-400:]
    assert strip_time(p.stdout) == strip_time(c.expected("stdout.txt"))
    for fn in FINALS:
        if os.path.exists(os.path.join(c.exp, fn)):
            assert c.got(fn) == c.expected(fn), fn
    for fn in os.listdir(os.path.join(c.exp, "tmp")):
        if fn == "_command.txt":            # the command line itself, with the options: what a --resume run reads
            assert c.got("tmp/" + fn) == c.expected("tmp/" + fn) + "".join(a + "\n" for a in extra).encode()
        else:
            assert c.got("tmp/" + fn) == c.expected("tmp/" + fn), fn
    want = model_region_gfa(c, 0, 100, 900, 1)
    assert want.count(b"\nS\t") > 0
    assert c.got("g.gfa") == want
    # only the named unit wrote lines, into a file named after the settings; the plain --graphOut names are not used
    parts = sorted(f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_graph."))
    assert parts == ["_graph.0.100-900.c1.gfa"]
    # --resume under another region (the argument file edited, the checkpoint rewound to the alignment): unit 0 is exported again under the new
    # settings, and the first run's lines, still in tmp/ under their own name, are not merged
    cmd = os.path.join(c.work, "tmp", "_command.txt")
    text = open(cmd).read()
    assert "0:100-900\n" in text
    with open(cmd, "w") as f:
        f.write(text.replace("0:100-900\n", "0:300-1400\n"))
    os.remove(os.path.join(c.work, "g.gfa"))
    with open(os.path.join(c.work, "tmp", "_checkpoint.txt"), "w") as f:
        f.write("0\n")
    p = c.run(cli, ["--resume"])
    assert p.returncode == 0 and b"RESUMED SUCCESSFULLY :-)" in p.stdout
    for fn in ("e.fa", "r.fa"):
        assert c.got(fn) == c.expected(fn), fn
    want2 = model_region_gfa(c, 0, 300, 1400, 1)
    assert want2 != want
    assert c.got("g.gfa") == want2
    parts = sorted(f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_graph."))
    assert parts == ["_graph.0.100-900.c1.gfa", "_graph.0.300-1400.c1.gfa"]


def usage_shown(p):
    return p.returncode == 255 and b"AlignGraph --read1" in p.stdout and b"Options:" in p.stdout


def test_region_options_need_graph_out_and_a_well_formed_region(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    assert usage_shown(c.run(cli, args + ["--graphRegion", "0:100-900"]))                                  # without --graphOut
    assert usage_shown(c.run(cli, args + ["--graphMinCoverage", "1"]))
    for bad in ("0:9-3", "x:1-2", "0:1", "0:-1-2", "0:1-2x", ":1-2", "0:1-", "0:01-2", "0:1-99999999999"):
        assert usage_shown(c.run(cli, args + ["--graphOut", "g.gfa", "--graphRegion", bad])), bad
    assert usage_shown(c.run(cli, args + ["--graphOut", "g.gfa", "--graphRegion", "0:1-2", "--graphRegion", "0:1-2"]))      # a second time
    assert usage_shown(c.run(cli, args + ["--graphOut", "g.gfa", "--graphMinCoverage", "-1"]))
    assert usage_shown(c.run(cli, args + ["--graphOut", "g.gfa", "--graphMinCoverage", "1", "--graphMinCoverage", "2"]))
    assert usage_shown(c.run(cli, args + ["--graphOut", "g.gfa", "--graphRegion"]))                        # no value
    # the reference's usage text does not name the options
    p = c.run(cli, args + ["--graphRegion", "0:1-2"])
    assert b"graphRegion" not in p.stdout and b"graphMinCoverage" not in p.stdout


def test_a_well_formed_region_is_accepted(cli, tmp_path):
    """Past the parser the run goes on as any other: here, without a device, up to the loud stop in front of the unit loop (with one, to the end)."""
    import aligngraph_amd as A
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a] + ["--graphOut", "g.gfa", "--graphRegion", "0:100-900", "--graphMinCoverage", "0"])
    assert b"(0) Alignment finished" in p.stdout and not usage_shown(p)
    if A.device_count() > 0:
        assert p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout
    else:
        assert p.returncode == 255 and b"NO HIP DEVICE" in p.stdout
    assert c.got("tmp/_command.txt").endswith(b"--graphOut\ng.gfa\n--graphRegion\n0:100-900\n--graphMinCoverage\n0\n")
