"""What the REAL reference binary did on the small runs that tests/test_oracle_golden.py and tests/test_rejected_inputs.py replay through it,
stored as data (tests/golden/reference_runs.json) so that those tests also hold where oracle/_ref is not built.

For every run the md5 of every input file (so that a test can tell "generator changed" from "engine differs") and what the reference made of
them: the md5 + length of its three per-unit output files (fresh_seed), or how it ended (rejected_inputs: crash / exit / finishes / hangs).
Where oracle/_ref is built the tests still run the reference live as well.

    python tests/golden/reference_runs.py          regenerate the table (needs oracle/_ref/AlignGraph_ref_O2)
"""
import hashlib
import json
import os
import pathlib
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "reference_runs.json")


def tree_md5(path):
    """{relative path: md5} of every file under `path`."""
    out = {}
    for d, _, files in os.walk(path):
        for fn in files:
            p = os.path.join(d, fn)
            with open(p, "rb") as f:
                out[os.path.relpath(p, path)] = hashlib.md5(f.read()).hexdigest()
    return dict(sorted(out.items()))


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import harness as H
    import test_oracle_golden as T1
    import test_rejected_inputs as T2
    H.build()
    if not H.have_reference(True):
        raise SystemExit("oracle/_ref is not built: the table records what the reference binary does")
    table = {"fresh_seed": None, "rejected_inputs": {}}
    with tempfile.TemporaryDirectory() as d:
        run = H.synth(os.path.join(d, "fresh"), **T1.FRESH_SEED)
        inputs = tree_md5(run)
        ref, _ = H.run_reference(run)
        table["fresh_seed"] = {"synth": T1.FRESH_SEED, "inputs_md5": inputs,
                               "expected": [{key: {"md5": hashlib.md5(o[key]).hexdigest(), "bytes": len(o[key])} for key in ("initial", "pre", "extended")} for o in ref]}
        for name in sorted(T2.CASES):
            where = pathlib.Path(d) / name
            where.mkdir()
            run = T2._run(where, name)
            inputs = tree_md5(run)
            table["rejected_inputs"][name] = {"inputs_md5": inputs, "reference": T2.reference_outcome(run)[0]}
            shutil.rmtree(where)
    with open(FIXTURE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
