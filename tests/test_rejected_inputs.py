"""The inputs the loader refuses (DESIGN.md "Rejected inputs"): what the product returns for each, and what the REFERENCE does with the same files.

Every class below is something bowtie2 / BLAT / formalizeGenome never produce, and on which the reference has no defined behaviour: it
indexes vectors out of bounds or carries state from one record into the next.  The product refuses each with a return code instead of
reproducing an accident.  The first half of every case runs everywhere (the loader is host code: the serial test executor links it); the
second half pins what the reference does — `crash` (killed by a signal), `exit` (its own error exit) or `finishes` — against the record of
the reference's runs on these very inputs (tests/golden/reference_runs.json), and against the reference binary itself where oracle/_ref is
built, so that a change of these expectations is a conscious edit of this table, and DESIGN.md can cite it.
"""
import os
import shutil
import subprocess

import pytest

import harness as H
from golden import reference_runs
from hostsim import sim

E_FORMAT, E_UNSUPPORTED = -2, -3


def _lines(path):
    with open(path) as f:
        return f.read().split("\n")


def _write(path, lines):
    with open(path, "w") as f:
        f.write("\n".join(lines))


def unsorted_sam(tmp):
    p = os.path.join(tmp, "_reads_genome.0.bowtie"); ln = _lines(p)
    ln[0:2], ln[2:4] = ln[2:4], ln[0:2]
    _write(p, ln)


def cigar_longer_than_read(tmp):
    p = os.path.join(tmp, "_reads_genome.0.bowtie"); ln = _lines(p)
    for i in (0, 1):
        t = ln[i].split("\t"); t[5] = "120M"; ln[i] = "\t".join(t)
    _write(p, ln)


def mates_not_adjacent(tmp):
    p = os.path.join(tmp, "_reads_genome.0.bowtie"); ln = _lines(p)
    ln[1], ln[2] = ln[2], ln[1]
    _write(p, ln)


def rname_of_another_unit(tmp):
    p = os.path.join(tmp, "_reads_genome.0.bowtie"); ln = _lines(p)
    for i in (0, 1):
        t = ln[i].split("\t"); t[2] = "3.1"; ln[i] = "\t".join(t)
    _write(p, ln)


def alignment_beyond_the_unit(tmp):
    p = os.path.join(tmp, "_reads_genome.0.bowtie"); ln = _lines(p)
    for i in (0, 1):
        t = ln[i].split("\t"); t[3] = str(8000 - 30 + 400 * i); t[5] = "100M"; ln[i] = "\t".join(t)
    _write(p, ln)


def two_records_in_the_unit_genome(tmp):
    p = os.path.join(tmp, "_genome.0.fa")
    with open(p, "a") as f:
        f.write(">1\nACGTACGTAC\n")


def empty_reads_file(tmp):
    open(os.path.join(tmp, "_reads.fa"), "w").close()


def psl_block_beyond_the_unit(tmp):
    p = os.path.join(tmp, "_contigs_genome.0.psl"); ln = _lines(p)
    t = ln[0].split("\t")
    starts = t[20].rstrip(",").split(","); starts[-1] = str(8000 - 5); t[20] = ",".join(starts) + ","
    ln[0] = "\t".join(t)
    _write(p, ln)


# name: (edit, product code, substring of the product's message, what the reference does)
CASES = {
    "unsorted_sam": (unsorted_sam, E_UNSUPPORTED, "not sorted by read id", "finishes"),      # the reference mixes the stale CIGAR segments of the skipped record into later reads (AG:1258): output, but not of these inputs
    "cigar_longer_than_read": (cigar_longer_than_read, E_UNSUPPORTED, "CIGAR length differs", "finishes"),      # it reads 20 bytes past the end of the read's vector: output, from memory that is not the input
    "mates_not_adjacent": (mates_not_adjacent, E_UNSUPPORTED, "", "crash"),
    "rname_of_another_unit": (rname_of_another_unit, E_UNSUPPORTED, "RNAME does not resolve", "crash"),
    "alignment_beyond_the_unit": (alignment_beyond_the_unit, E_UNSUPPORTED, "beyond the end of the unit", "crash"),
    "two_records_in_the_unit_genome": (two_records_in_the_unit_genome, E_UNSUPPORTED, "more than one record", "finishes"),
    "empty_reads_file": (empty_reads_file, E_FORMAT, "no pairs", "crash"),
    "psl_block_beyond_the_unit": (psl_block_beyond_the_unit, E_FORMAT, "beyond the unit", "finishes"),      # positions past the end of genome[0]: a write through an out-of-range index that happens not to fault here
}


def _run(tmp_path, name):
    run = H.synth(str(tmp_path / "run"), seed=61, chroms="8000", pairs=1500, coverage=3, multi=0, read_indel=0, read_clip=0, read_badclip=0, unaligned=0,
                  contig_min=1500, contig_max=3000, contig_split=0, contig_dup=0, contig_overlap=0, contig_lowid=0, sam_seq=0)
    CASES[name][0](os.path.join(run, "tmp"))
    return run


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_loader_refuses_with_a_code(built, tmp_path, name):
    run = _run(tmp_path, name)
    _, code, msg, _ = CASES[name]
    if name == "alignment_beyond_the_unit":
        pytest.skip("decided on the device (agx_k_hit_prep: the arrival span of a hit ends beyond the unit): tests/test_gpu_parity.py::test_error_codes")
    with pytest.raises(sim.SimError) as e:
        sim.run(os.path.join(run, "tmp"), 0, k=5, insert_variation=50, coverage=3)
    assert e.value.code == code and msg in e.value.msg, (e.value.code, e.value.msg)


def reference_outcome(run):
    """Replays a copy of `run` through the reference binary: "crash", "exit", "finishes" or "hangs", and the tail of its stdout."""
    work = run + ".ref"
    shutil.copytree(run, work)
    env = dict(os.environ, PATH=H.STUBS + os.pathsep + os.environ.get("PATH", ""))
    try:
        p = subprocess.run([H.REF_O2, "--resume"], cwd=work, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        return "crash" if p.returncode < 0 else "finishes" if p.returncode == 0 and b"FINISHED SUCCESSFULLY" in p.stdout else "exit", p.stdout[-200:]
    except subprocess.TimeoutExpired:
        return "hangs", b""


@pytest.mark.parametrize("name", sorted(CASES))
def test_what_the_reference_does_with_them(built, tmp_path, name):
    """Against what the reference did with these very inputs (tests/golden/reference_runs.json), and against the reference itself where oracle/_ref is built."""
    run = _run(tmp_path, name)
    rec = reference_runs.load()["rejected_inputs"][name]
    assert reference_runs.tree_md5(run) == rec["inputs_md5"], "the generator no longer reproduces the inputs the reference was run on: regenerate tests/golden/reference_runs.json"
    assert rec["reference"] == CASES[name][3], "%s: the reference %s" % (name, rec["reference"])
    if H.have_reference():
        got, tail = reference_outcome(run)
        assert got == CASES[name][3], "%s: the reference %s (stdout tail: %r)" % (name, got, tail)
