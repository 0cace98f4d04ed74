"""AlignGraph_amd --graphOut with --graphPaths: the end-to-end cases of test_cli_graph.py with the records of every unit laid over its segments.  Everything the
reference writes stays byte for byte as it is; g.gfa is the GFA header followed, unit by unit, by the model's S and L lines and the path model's P lines
(tests/path_model.py on the oracle's graph, over the stretches the library keeps for the same unit); without --graphPaths the run writes what it wrote before the option
existed.  Without --graphOut the option prints usage like every other malformed option."""
import os

import pytest

import harness as H
import path_model as PM
import unitig_model as M
import unitig_region_model as R
import walk_model as WM
from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)
from test_cli_graph import option


def model_gfa(c, region, min_cov):
    """The expected g.gfa with and without P lines."""
    import aligngraph_amd as A
    k, iv, cov = option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)
    tmp = os.path.join(c.work, "tmp")
    plain, paths = [M.GFA_HEADER], [M.GFA_HEADER]
    for unit in range(c.units):
        if region is not None and unit != region[0]:
            continue
        o = H.run_oracle(tmp, unit, k, iv, cov, graph=True)
        g = o["graph"]
        lo, hi = (region[1], region[2]) if region is not None else (0, g["n_pos"])
        mc = cov if min_cov is None else min_cov
        sl = R.region_gfa(g, lo, hi, mc, M.read_reference(tmp, unit), unit)
        with A.Unit(k=k, insert_variation=iv, coverage=cov, keep_paths=True) as u:      # the stretches: what the walk did is the library's to say (tests/test_gpu_paths.py holds them against the oracle)
            u.load_files(tmp, unit)
            u.upload()
            u.build()
            assert u.finish()["pre"] == o["pre"]
            w = u.walk_paths()
        mu, es, er = PM.id_map(g, cov, lo, hi, mc, bytes(g["pos_nuc"]), WM.build(g, cov))
        assert M.gfa_text(mu, unit) == sl
        plain.append(sl)
        paths.append(sl + PM.paths_gfa(mu, es, er, w, unit))
    return b"".join(plain), b"".join(paths)


@pytest.mark.gpu
@pytest.mark.parametrize("window", [[], ["--graphRegion", "0:100-900", "--graphMinCoverage", "1"]])
def test_graph_paths(cli, built, window, tmp_path):
    c = Case("default", tmp_path / "with")
    extra = ["--graphOut", "g.gfa"] + window + ["--graphPaths"]
    p = c.run(cli, [a for a in c.args if a] + extra)
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
    plain, paths = model_gfa(c, (0, 100, 900) if window else None, 1 if window else None)
    assert paths.count(b"\nP\t") > 0 and plain.count(b"\nS\t") > 0
    assert c.got("g.gfa") == paths
    # the same run without the option: the file of before
    d = Case("default", tmp_path / "without")
    p = d.run(cli, [a for a in d.args if a] + ["--graphOut", "g.gfa"] + window)
    assert p.returncode == 0, p.stdout[-400:]
    assert d.got("g.gfa") == plain
    for fn in os.listdir(os.path.join(d.work, "tmp")):
        if fn.startswith("_graph."):
            assert b"\nP\t" not in d.got("tmp/" + fn)


def test_graph_paths_needs_graph_out(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    for bad in (["--graphPaths"], ["--graphOut", "g.gfa", "--graphPaths", "--graphPaths"]):
        p = c.run(cli, args + bad)
        assert p.returncode == 255 and b"AlignGraph --read1" in p.stdout and b"Options:" in p.stdout and b"graphPaths" not in p.stdout


def test_graph_paths_is_accepted(cli, tmp_path):
    """Past the parser the run goes on as any other: here, without a device, up to the loud stop in front of the unit loop (with one, to the end)."""
    import aligngraph_amd as A
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a] + ["--graphOut", "g.gfa", "--graphPaths"])
    assert b"(0) Alignment finished" in p.stdout
    if A.device_count() > 0:
        assert p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout
    else:
        assert p.returncode == 255 and b"NO HIP DEVICE" in p.stdout
    assert c.got("tmp/_command.txt").endswith(b"--graphOut\ng.gfa\n--graphPaths\n")
