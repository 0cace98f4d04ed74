"""AlignGraph_amd --linksOut: the end-to-end case of test_cli.py with the links between every unit's pre-extended records written as TSV.  Everything the reference
writes stays byte for byte as it is; the file is, unit by unit, the mate-links model's text (tests/links_model.py on the serial executor's front and the walk model's side
positions, over the stretches the library keeps for the same unit) at the run's threshold; the per-unit files in tmp/ carry the threshold in their names; a --resume that
redoes the last unit gives the same file; the option combines with --evidenceOut and --spanOut, whose files stay what they are without it; without the option the run
writes what it wrote before the option existed.  The threshold option alone prints usage."""
import os

import pytest

import harness as H
import links_model as LM
import span_model as SM
import walk_model as WM
from hostsim import sim
from test_cli import FINALS, Case, cli, strip_time  # noqa: F401  (cli: the module fixture)
from test_cli_evidence import model_beds
from test_cli_graph import option
from test_cli_span import model_span_beds


def model_links(c, min_pairs):
    """The expected per-unit TSV texts."""
    import aligngraph_amd as A
    k, iv, cov = option(c.args, "--kMer", 5), option(c.args, "--insertVariation", 50), option(c.args, "--coverage", 20)
    tmp = os.path.join(c.work, "tmp")
    out = []
    for unit in range(c.units):
        o = H.run_oracle(tmp, unit, k, iv, cov, graph=True)
        front = sim.run(tmp, unit, k, iv, cov, front=True)["front"]
        with A.Unit(k=k, insert_variation=iv, coverage=cov, keep_paths=True) as u:      # the stretches: what the walk did is the library's to say (tests/test_gpu_paths.py holds them against the oracle)
            u.load_files(tmp, unit)
            u.upload()
            u.build()
            assert u.finish()["pre"] == o["pre"]
            w = u.walk_paths()
        l = LM.mate_links(SM.fragments(front), int(front["n_pos"]), WM.build(o["graph"], cov)["side_xpos"], w, min_pairs)
        assert LM.identity(l)
        out.append(LM.tsv(l, unit))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [[], ["--linksMin", "1"]])
def test_links_out(cli, built, threshold, tmp_path):
    c = Case("default", tmp_path / "with")
    extra = ["--linksOut", "links.tsv"] + threshold
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
    mp = 1 if threshold else 2
    texts = model_links(c, mp)
    parts = ["_links.%d.m%d.tsv" % (u, mp) for u in range(c.units)]
    assert sorted(f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_links.")) == sorted(parts)
    for fn, text in zip(parts, texts):
        assert c.got("tmp/" + fn) == text, fn
    assert c.got("links.tsv") == b"".join(texts)
    assert all(line.count(b"\t") == 7 and line.startswith(b"p") for line in c.got("links.tsv").splitlines())
    # --resume that redoes the last unit: its outputs and its links file removed, the checkpoint rewound
    last = c.units - 1
    for stem in ("_initial_contigs", "_pre_extended_contigs", "_extended_contigs"):
        os.remove(os.path.join(c.work, "tmp", "%s.%d.fa" % (stem, last)))
    os.remove(os.path.join(c.work, "tmp", parts[last]))
    os.remove(os.path.join(c.work, "links.tsv"))
    with open(os.path.join(c.work, "tmp", "_checkpoint.txt"), "w") as f:
        f.write("0\n%d\n" % last)
    p = c.run(cli, ["--resume"])
    assert p.returncode == 0 and b"RESUMED SUCCESSFULLY :-)" in p.stdout
    assert c.got("links.tsv") == b"".join(texts) and c.got("tmp/" + parts[last]) == texts[last]
    for fn in ("e.fa", "r.fa"):
        assert c.got(fn) == c.expected(fn), fn


@pytest.mark.gpu
def test_combined_with_evidence_out_and_span_out(cli, built, tmp_path):
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a] + ["--evidenceOut", "weak.bed", "--spanOut", "thin.bed", "--spanMin", "3", "--linksOut", "links.tsv", "--linksMin", "1"])
    assert p.returncode == 0, p.stdout[-400:]
    assert strip_time(p.stdout) == strip_time(c.expected("stdout.txt"))
    for fn in FINALS:
        if os.path.exists(os.path.join(c.exp, fn)):
            assert c.got(fn) == c.expected(fn), fn
    assert c.got("links.tsv") == b"".join(model_links(c, 1))
    assert c.got("thin.bed") == b"".join(model_span_beds(c, 3))
    assert c.got("weak.bed") == b"".join(model_beds(c, None, None))


@pytest.mark.gpu
def test_without_the_option_nothing_new_is_written(cli, tmp_path):
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a])
    assert p.returncode == 0, p.stdout[-400:]
    assert strip_time(p.stdout) == strip_time(c.expected("stdout.txt"))
    assert not [f for f in os.listdir(os.path.join(c.work, "tmp")) if f.startswith("_links.")]
    for fn in os.listdir(os.path.join(c.exp, "tmp")):
        assert c.got("tmp/" + fn) == c.expected("tmp/" + fn), fn
    assert not [f for f in os.listdir(c.work) if f.endswith(".tsv")]


def test_threshold_needs_links_out(cli, tmp_path):
    c = Case("default", tmp_path)
    args = [a for a in c.args if a]
    for bad in (["--linksMin", "3"], ["--linksOut", "t.tsv", "--linksMin", "-1"], ["--linksOut", "t.tsv", "--linksMin", "2x"], ["--linksOut", "t.tsv", "--linksOut", "v.tsv"],
                ["--linksOut"]):
        p = c.run(cli, args + bad)
        assert p.returncode == 255 and b"AlignGraph --read1" in p.stdout and b"Options:" in p.stdout and b"links" not in p.stdout, bad


def test_links_out_is_accepted(cli, tmp_path):
    """Past the parser the run goes on as any other: here, without a device, up to the loud stop in front of the unit loop (with one, to the end)."""
    import aligngraph_amd as A
    c = Case("default", tmp_path)
    p = c.run(cli, [a for a in c.args if a] + ["--linksOut", "links.tsv", "--linksMin", "3"])
    assert b"(0) Alignment finished" in p.stdout
    if A.device_count() > 0:
        assert p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout
        assert os.path.exists(os.path.join(c.work, "tmp", "_links.0.m3.tsv"))
    else:
        assert p.returncode == 255 and b"NO HIP DEVICE" in p.stdout
    assert c.got("tmp/_command.txt").endswith(b"--linksOut\nlinks.tsv\n--linksMin\n3\n")
