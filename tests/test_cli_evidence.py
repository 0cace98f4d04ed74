"""AlignGraph_amd --evidenceOut: the end-to-end case of test_cli.py with the weak intervals of every unit's pre-extended records written as BED.  Everything the
reference writes stays byte for byte as it is; the file is, unit by unit, the evidence model's text (tests/evidence_model.py on the oracle's graph and the edge-support
model, over the stretches the library keeps for the same unit) at the run's thresholds; the per-unit files in tmp/ carry the thresholds in their names; a --resume that
redoes the last unit gives the same file; without the option the run writes what it wrote before the option existed.  The threshold options alone print usage."""
import os

import pytest

import edge_support_model as ESM
import evidence_model as EM
import harness as H
import walk_model as WM
from hostsim import sim
from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)
from test_cli_graph import option


def model_beds(c, min_depth, min_support):
    """The expected per-unit BED texts."""
    import aligngraph_amd as A
    k, iv, cov = option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)
    tmp = os.path.join(c.work, "tmp")
    out = []
    for unit in range(c.units):
        o = H.run_oracle(tmp, unit, k, iv, cov, graph=True)
        g = o["graph"]
        sup = ESM.support(sim.run(tmp, unit, k, iv, cov, front=True)["front"], g, k, iv)
        with A.Unit(k=k, insert_variation=iv, coverage=cov, keep_paths=True) as u:      # the stretches: what the walk did is the library's to say (tests/test_gpu_paths.py holds them against the oracle)
            u.load_files(tmp, unit)
            u.upload()
            u.build()
            assert u.finish()["pre"] == o["pre"]
            w = u.walk_paths()
        e = EM.evidence(g, cov, w, sup, cov if min_depth is None else min_depth, 2 if min_support is None else min_support, wm=WM.build(g, cov))
        out.append(EM.bed(e, unit))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("thresholds", [[], ["--evidenceMinDepth", "1000000", "--evidenceMinSupport", "6"]])
def test_evidence_out(cli, built, thresholds, tmp_path):
    c = Case("default", tmp_path / "with")
    extra = ["--evidenceOut", "weak.bed"] + thresholds
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
    cov = option(c.args, "--coverage", 20)
    md, ms = (1000000, 6) if thresholds else (cov, 2)
    beds = model_beds(c, md if thresholds else None, ms if thresholds else None)
    parts = ["_evidence.%d.d%d.s%d.bed" % (u, md, ms) for u in range(c.units)]
    assert sorted(f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_evidence.")) == sorted(parts)
    for fn, text in zip(parts, beds):
        assert c.got("tmp/" + fn) == text, fn
    assert c.got("weak.bed") == b"".join(beds)
    if thresholds:
        assert c.got("weak.bed").count(b"\n") >= b"".join(c.got("tmp/_pre_extended_contigs.%d.fa" % u) for u in range(c.units)).count(b">") > 0      # (above every depth every record is weak from its first graph base on)
    # --resume that redoes the last unit: its outputs and its evidence file removed, the checkpoint rewound
    last = c.units - 1
    for stem in ("_initial_contigs", "_pre_extended_contigs", "_extended_contigs"):
        os.remove(os.path.join(c.work, "tmp", "%s.%d.fa" % (stem, last)))
    os.remove(os.path.join(c.work, "tmp", parts[last]))
    os.remove(os.path.join(c.work, "weak.bed"))
    with open(os.path.join(c.work, "tmp", "_checkpoint.txt"), "w") as f:
        f.write("0\n%d\n" % last)
    p = c.run(cli, ["--resume"])
    assert p.returncode == 0 and b"RESUMED SUCCESSFULLY :-)" in p.stdout
    assert c.got("weak.bed") == b"".join(beds) and c.got("tmp/" + parts[last]) == beds[last]
    for fn in ("e.fa", "r.fa"):
        assert c.got(fn) == c.expected(fn), fn


@pytest.mark.gpu
def test_without_the_option_nothing_new_is_written(cli, tmp_path):
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a])
    assert p.returncode == 0, p.stdout[-400:]
    assert not [f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_evidence.")]
    assert not [f for f in os.listdir(c.work) if f.endswith(".bed")]


def test_thresholds_need_evidence_out(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    for bad in (["--evidenceMinDepth", "3"], ["--evidenceMinSupport", "3"], ["--evidenceOut", "w.bed", "--evidenceMinDepth", "-1"], ["--evidenceOut", "w.bed", "--evidenceMinSupport", "2x"],
                ["--evidenceOut", "w.bed", "--evidenceOut", "v.bed"], ["--evidenceOut"]):
        p = c.run(cli, args + bad)
        assert p.returncode == 255 and b"AlignGraph --read1" in p.stdout and b"Options:" in p.stdout and b"evidence" not in p.stdout, bad


def test_evidence_out_is_accepted(cli, tmp_path):
    """Past the parser the run goes on as any other: here, without a device, up to the loud stop in front of the unit loop (with one, to the end)."""
    import aligngraph_amd as A
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a] + ["--evidenceOut", "weak.bed", "--evidenceMinSupport", "3"])
    assert b"(0) Alignment finished" in p.stdout
    if A.device_count() > 0:
        assert p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout
        assert os.path.exists(os.path.join(c.work, "tmp", "_evidence.0.d%d.s3.bed" % option(c.args, "--coverage", 20)))
    else:
        assert p.returncode == 255 and b"NO HIP DEVICE" in p.stdout
    assert c.got("tmp/_command.txt").endswith(b"--evidenceOut\nweak.bed\n--evidenceMinSupport\n3\n")
