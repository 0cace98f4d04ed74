"""What the REAL reference binary wrote for every hand-made unit of the suite, stored as data (tests/golden/hand_units_reference.json) so that
tests/test_hand_units_reference.py holds the oracle and the serial executor against the reference itself on every one of them — the units of
tests/window_units.py, which sit on the edges of the compatibility windows, among them — also where oracle/_ref is not built.

For every case of lean_units, edge_units, walk_units, sweep_units, front_units, unitig_units and window_units, at the case's coverage and at every
coverage it names for a reprune: the md5 of each input file (so that a test can tell "the unit changed" from "the engine differs") and the md5 and
length of the reference's three output files.  The run directory is what tools/agx_synth writes: tmp/_command.txt and tmp/_checkpoint.txt, empty
reads_1.fa / reads_2.fa, and contigs.fa / genome.fa (without the last two the reference prints its usage and exits), replayed with
harness.run_reference.  The unoptimised and the optimised build of the reference must agree (as tests/golden/make_golden.py asserts).

    python tests/golden/make_hand_units_reference.py          regenerate the table (needs oracle/_ref)
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "hand_units_reference.json")
KEYS = ("initial", "pre", "extended")
COMMAND = ("--read1\nreads_1.fa\n--read2\nreads_2.fa\n--contig\ncontigs.fa\n--genome\ngenome.fa\n--distanceLow\n100\n--distanceHigh\n1500\n"
           "--extendedContig\nextended.fa\n--remainingContig\nremaining.fa\n--kMer\n%d\n--coverage\n%d\n--insertVariation\n%d\n--part\n1\n")


class HandUnit:
    def __init__(self, name, write, iv, coverages, refused=False):
        """write(run) -> the unit's tmp/ directory; coverages: the case's own first, then those it names for a reprune; refused: the engine refuses the unit by design
        (sweep_units' overflow case: more variants at a position than its widest bucket holds) — the reference and the oracle still answer"""
        self.name, self.write, self.iv, self.coverages, self.refused = name, write, iv, list(dict.fromkeys(coverages)), refused


def units():
    """Every hand-made unit of the suite, in a fixed order."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_units as EU
    import front_units as FU
    import lean_units as LU
    import sweep_units as SU
    import unitig_units as UU
    import walk_units as WU
    import window_units as XU
    out = [HandUnit("lean:" + c.name, lambda d, c=c: LU.write_unit(c.unit, d), LU.IV, [1]) for c in LU.cases()]
    out += [HandUnit("edge:" + c.name, lambda d, c=c: LU.write_unit(c.unit, d), c.iv, [c.coverage]) for c in EU.cases()]
    out += [HandUnit("walk:" + c.name, lambda d, c=c: WU.write_unit(c.unit, d), c.iv, [c.coverage]) for c in WU.cases()]
    out += [HandUnit("sweep:" + c.name, lambda d, c=c: c.write(d), c.iv, [c.coverage], refused=c.overflow) for c in SU.cases()]
    out += [HandUnit("front:" + c.name, lambda d, c=c: FU.write_unit(c, d), LU.IV, [1]) for c in FU.cases()]
    out += [HandUnit("unitig:" + c.name, lambda d, c=c: WU.write_unit(c.unit, d), c.iv, [c.coverage] + list(c.reprune)) for c in UU.cases()]
    out += [HandUnit("window:" + c.name, lambda d, c=c: c.write(d), c.iv, [c.coverage] + list(c.reprune)) for c in XU.cases()]
    assert len({u.name for u in out}) == len(out)
    return out


K = 5      # every hand-made unit runs with k = 5 (lean_units.K)


def inputs_md5(tmp):
    out = {}
    for fn in sorted(os.listdir(tmp)):
        with open(os.path.join(tmp, fn), "rb") as f:
            out[fn] = hashlib.md5(f.read()).hexdigest()
    return out


def prepare_run(run, tmp, iv, coverage):
    """Makes `run` (whose tmp/ holds a unit's files) a directory the reference resumes from."""
    with open(os.path.join(tmp, "_command.txt"), "w") as f:
        f.write(COMMAND % (K, coverage, iv))
    with open(os.path.join(tmp, "_checkpoint.txt"), "w") as f:
        f.write("0\n")
    for fn in ("reads_1.fa", "reads_2.fa"):
        open(os.path.join(run, fn), "w").close()
    shutil.copy(os.path.join(tmp, "_contigs.fa"), os.path.join(run, "contigs.fa"))
    shutil.copy(os.path.join(tmp, "_genome.0.fa"), os.path.join(run, "genome.fa"))


def run_reference(H, run, tmp, iv, coverage, opt=True):
    prepare_run(run, tmp, iv, coverage)
    try:
        outs, _ = H.run_reference(run, opt=opt)
    finally:
        for fn in ("_command.txt", "_checkpoint.txt"):
            os.remove(os.path.join(tmp, fn))
    assert len(outs) == 1
    return outs[0]


def digest(out):
    return {key: {"md5": hashlib.md5(out[key]).hexdigest(), "bytes": len(out[key])} for key in KEYS}


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import harness as H
    H.build()
    if not (H.have_reference(True) and H.have_reference(False)):
        raise SystemExit("oracle/_ref is not built: the table records what the reference binary does")
    table = {}
    for u in units():
        with tempfile.TemporaryDirectory() as d:
            run = os.path.join(d, "run")
            tmp = u.write(run)
            rec = {"insert_variation": u.iv, "inputs_md5": inputs_md5(tmp), "expected": {}}
            for cov in u.coverages:
                o2, o0 = run_reference(H, run, tmp, u.iv, cov, True), run_reference(H, run, tmp, u.iv, cov, False)
                assert o0 == o2, "%s at coverage %d: the reference's -O0 and -O2 builds differ" % (u.name, cov)
                rec["expected"][str(cov)] = digest(o2)
            table[u.name] = rec
            print("%-36s %s" % (u.name, " ".join("%s:%d" % (c, sum(v["bytes"] for v in e.values())) for c, e in rec["expected"].items())), flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE, "-", len(table), "units,", sum(len(r["expected"]) for r in table.values()), "runs")


if __name__ == "__main__":
    main()
