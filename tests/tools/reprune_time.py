#!/usr/bin/env python3
"""What a change of coverage costs on a resident 30.4 Mb unit (the unit of the full-size export tests), three ways, alternating three times in one process after a
warm-up of each: reprune 5 -> 20 -> 5 (agx_stats ms_reprune of each call), build() on the same resident unit (wall), and the change done without agx_unit_reprune: a new
Unit at 20, load_files from the unit cache, upload, build (wall).  Prints the minimum and all three values of each, and checks that finish() after the reprune and
finish() of the fresh unit are the same bytes.  Not a test: nothing here asserts a time.
Usage (GPU box): python tests/tools/reprune_time.py [--work DIR]      (under rocprofv3 --kernel-trace --stats for agx_k_reprune beside agx_k_assign_aid / agx_k_emit_alive)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import harness as H          # noqa: E402
import aligngraph_amd as A   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--work", default="/tmp/agx_reprune_time")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

run = H.synth(a.work, seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
tmp = os.path.join(run, "tmp")
A.cache_build(tmp, 0)


def ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def fresh(cov):
    u = A.Unit(k=5, insert_variation=50, coverage=cov, keep_counts=True)
    u.load_files(tmp, 0)
    u.upload()
    u.build()
    return u


def fresh_at_20():
    fresh(20).close()


u = fresh(5)
print("unit: %d positions, %d nodes, from_cache %d" % (u.stats()["n_pos"], u.stats()["n_nodes"], u.stats()["from_cache"]), flush=True)
u.reprune(20); u.reprune(5); u.build(); fresh_at_20()      # warm-up of each form
up, down, rebuild, anew = [], [], [], []
for _ in range(a.rounds):
    u.reprune(20); up.append(u.stats()["ms_reprune"])
    u.reprune(5); down.append(u.stats()["ms_reprune"])
    rebuild.append(ms(u.build))
    anew.append(ms(fresh_at_20))
for name, v in (("reprune 5 -> 20 (ms_reprune)", up), ("reprune 20 -> 5 (ms_reprune)", down), ("build() on the resident unit (wall)", rebuild),
                ("new Unit at 20: load_files from the cache, upload, build (wall)", anew)):
    print("%-66s min %8.3f ms   all %s" % (name, min(v), " ".join("%.3f" % x for x in v)), flush=True)
u.reprune(20)
print("reprune_attempts of the last call: %d" % u.stats()["reprune_attempts"])
got = u.finish()
with fresh(20) as f:
    want = f.finish()
same = all(got[k] == want[k] for k in ("initial", "pre", "extended"))
print("finish() after reprune(20) == finish() of a fresh unit at 20: %s (%d / %d / %d bytes)" % (same, len(got["initial"]), len(got["pre"]), len(got["extended"])))
u.close()
sys.exit(0 if same else 1)
