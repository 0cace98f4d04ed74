#!/usr/bin/env python3
"""Mutation check of the content rules (aligngraph_amd/csrc/agx_load.cpp "content rules"): every clause removed in turn, on a scratch copy of the sources, CPU only.

    python tests/tools/damaged_inputs_mutations.py <scratch dir> [jobs]

A clause is one `return "<rule>"` (or `bad[t] = "<rule>"`) with its condition; where the condition is several clauses joined by `||`, each of them in turn is made false.
Per mutant the serial executor's library is built from the mutated loader and tests/test_damaged_inputs.py's table tests run against it (AGX_HOSTSIM_LIB); if the table
does not notice, tests/damaged_inputs_san.cpp is built from it too and run.  Prints one line per mutant: the clause, and what caught it (profiles/damaged_inputs_mutations.txt
is this output)."""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "aligngraph_amd", "csrc")
SMALL = None


def top_level_or(cond):
    parts, depth, at = [], 0, 0
    for i, ch in enumerate(cond):
        depth += ch == "("
        depth -= ch == ")"
        if depth == 0 and cond.startswith("||", i):
            parts.append(cond[at:i])
            at = i + 2
    return parts + [cond[at:]]


def mutants(src):
    lo, hi = src.index("const char *pairs_header_rule("), src.index("build_cm_layout(const agx_u8 *cm_cnt")
    for m in re.finditer(r'return "(\w+)";|bad\[t\] = "(\w+)"; return;', src[lo:hi]):
        site, rule = lo + m.start(), m.group(1) or m.group(2)
        stmt = "(void)0;" if m.group(1) else ""
        removed = src[:site] + stmt + src[lo + m.end():]
        # the condition in front of it: the nearest `if (` on the same line
        line0 = src.rfind("\n", 0, site) + 1
        i = src.rfind("if (", line0, site)
        cond = None
        if i >= 0:
            depth, j = 0, i + 3
            for j in range(i + 3, site):
                depth += src[j] == "("
                depth -= src[j] == ")"
                if depth == 0:
                    break
            cond = src[i + 4:j]
        clauses = top_level_or(cond) if cond else [None]
        line = src.count("\n", 0, site) + 1
        if len(clauses) == 1:
            yield "%s (line %d): %s" % (rule, line, (cond or "").strip()), removed
        else:
            for c in clauses:
                k = src.index(c, i)
                yield "%s (line %d): clause %s" % (rule, line, c.strip()), src[:k] + " false " + src[k + len(c):]


def run_one(args):
    n, what, text, scratch = args
    d = os.path.join(scratch, "m%03d" % n)
    shutil.rmtree(d, ignore_errors=True)
    shutil.copytree(os.path.join(ROOT, "aligngraph_amd", "csrc"), os.path.join(d, "aligngraph_amd", "csrc"))
    os.makedirs(os.path.join(d, "tests"))
    for f in ("hostsim", "damaged_inputs_san.cpp", "wire_shim.cpp"):
        s = os.path.join(ROOT, "tests", f)
        (shutil.copytree if os.path.isdir(s) else shutil.copy)(s, os.path.join(d, "tests", f))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
    c = os.path.join(d, "aligngraph_amd", "csrc")
    with open(os.path.join(c, "agx_load.cpp"), "w") as f:
        f.write(text)
    src = [os.path.join(c, x) for x in ("agx_host.cpp", "agx_walk.cpp", "agx_load.cpp")]
    lib = os.path.join(d, "libagx_hostsim.so")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-w", "-o", lib, os.path.join(d, "tests", "hostsim", "agx_hostsim.cpp")] + src, capture_output=True, text=True)
    if r.returncode:
        return n, what, "does not compile: " + r.stderr.strip().split("\n")[0]
    env = dict(os.environ, AGX_HOSTSIM_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_damaged_inputs.py"), "-k", "small_unit or entry_gives"],
                       capture_output=True, text=True, env=env, cwd=ROOT)
    if r.returncode:
        first = [ln for ln in r.stdout.split("\n") if ln.startswith("FAILED") or ln.startswith("ERROR")]
        msg = [ln for ln in r.stdout.split("\n") if ln.startswith("E   ") and "Error" in ln]
        return n, what, "table: " + (first[0].split("::")[-1] if first else "?") + (" — " + msg[0][4:].strip() if msg else "")
    exe = os.path.join(d, "san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread", "-w", "-o", exe, os.path.join(d, "tests", "damaged_inputs_san.cpp")] + src,
                       capture_output=True, text=True)
    if r.returncode:
        return n, what, "sanitizer program does not compile"
    r = subprocess.run([exe, SMALL, "0", "5", "2000", "1"], capture_output=True, text=True)
    if r.returncode:
        err = [ln for ln in r.stderr.split("\n") if "ERROR" in ln or "runtime error" in ln or "refused" in ln or "mutant" in ln]
        where = [ln.strip() for ln in r.stderr.split("\n") if ln.strip().startswith("#0") or ln.strip().startswith("#1")]
        return n, what, "sanitizer program (exit %d): %s %s" % (r.returncode, err[0].strip()[:160] if err else "", " / ".join(w[:120] for w in where[:2]))
    return n, what, "NOTHING: the table passes and the sanitizer program exits 0 (%s)" % r.stdout.strip().split("\n")[-1]


def main():
    global SMALL
    scratch = os.path.abspath(sys.argv[1])
    jobs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import harness as H
    from test_damaged_inputs import SMALL as kw
    SMALL = os.path.join(H.synth(os.path.join(scratch, "small", "run"), **kw), "tmp")
    src = open(os.path.join(CSRC, "agx_load.cpp")).read()
    work = [(n, what, text, scratch) for n, (what, text) in enumerate(mutants(src))]
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for n, what, got in ex.map(run_one, work):
            print("%3d | %s | %s" % (n, what, got), flush=True)
            shutil.rmtree(os.path.join(scratch, "m%03d" % n), ignore_errors=True)


if __name__ == "__main__":
    main()
