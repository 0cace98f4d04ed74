#!/usr/bin/env python3
"""What the mate links cost on a resident 30.4 Mb unit (the unit of the full-size export tests) at coverage 5 after a finish, in one process:
  - the call's own time (agx_mate_links.ms, "ms" below) of Unit.mate_links() on the table of the unit's own finish at min_pairs 2, `rounds` times after a warm-up, with the wall time of the
    Python call, and once more at min_pairs 1;
  - the passes, slots, distinct keys and load of the table, the kept links, the totals of the classes;
  - once with the slot count forced to a quarter of the distinct keys (rounded up to a power of two): the ranges are halved, every pass one more read of all hits;
  - for comparison in the same trace, one Unit.pair_span() (agx_k_span_mark: the same loop over the hits with two adds per hit);
  - the device against tests/links_model.py on the fragments of the front Unit.front() copies out (tests/span_wide.py makes them, fast at this size) and the side
    positions of Unit.walk_graph(), asked last;
  - consistency: the identity over the totals, the forced call equals the plain one, a finish behind it all gives the same bytes.
Prints every value.  Not a test: nothing here asserts a time.
Usage (GPU box): python tests/tools/links_time.py [--work DIR] [--rounds N] [--no-model]      (under rocprofv3 --kernel-trace --stats for the kernels of agx_links.hip;
AGX_LIB_PATH=<variant library> for an A/B of two builds, same box, alternating)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness as H          # noqa: E402
import aligngraph_amd as A   # noqa: E402
import links_model as LM     # noqa: E402
import span_wide as SW       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--work", default="/tmp/agx_links_time")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--no-model", action="store_true")
a = ap.parse_args()

run = H.synth(a.work, seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
tmp = os.path.join(run, "tmp")
A.cache_build(tmp, 0)


def ms(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def line(name, v):
    print("%-78s min %10.3f ms   all %s" % (name, min(v), " ".join("%.3f" % x for x in v)), flush=True)


print("library: %s" % A.LIB_PATH, flush=True)
u = A.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True, keep_paths=True)
u.load_files(tmp, 0)
need = u.hbm_needed()
u.upload()
u.build()
t_fin, fin = ms(u.finish)
w = u.walk_paths()
st = u.stats()
print("unit: %d positions, %d hits, %d runs, %d nodes, %d walk ids; hbm_needed %d; finish %.1f ms; device_bytes %d" %
      (st["n_pos"], st["n_hits"], st["n_runs"], st["n_nodes"], st["n_walk_ids"], need, t_fin, st["device_bytes"]), flush=True)
first = u.mate_links(w, 2)
s1 = u.stats()
print("first call: ms %.3f; device_bytes %d" % (first["ms"], s1["device_bytes"]), flush=True)
print("table of the finish: %d records, %d stretches; %d owned positions, %d shadowed graph bases" % (len(w["rec_len"]), len(w["id_first"]), first["n_owned"], first["n_shadowed"]), flush=True)
print("mate links: %d passes, %d slots, %d distinct keys (load %.6f), %d kept links at min_pairs 2" %
      (first["n_passes"], first["n_slots"], first["n_links_all"], first["n_links_all"] / first["n_slots"], len(first["a"])), flush=True)
print("classes: %d kept hits, %d outside, %d fragments = %d unowned + %d inside + %d open + %d link pairs; the identity holds: %s; most pairs on one link %d" %
      (first["n_kept"], first["n_outside"], first["n_fragments"], first["n_unowned"], first["n_inside"], first["n_open"], first["n_link_pairs"], LM.identity(first),
       int(first["n_pairs"].max()) if len(first["n_pairs"]) else 0), flush=True)
stat, wall = [], []
for _ in range(a.rounds):
    t, r = ms(lambda: u.mate_links(w, 2))
    wall.append(t)
    stat.append(r["ms"])
line("agx_mate_links.ms, the finish's table, min_pairs 2", stat)
line("Unit.mate_links(), wall time of the Python call", wall)
every = u.mate_links(w, 1)
print("at min_pairs 1: ms %.3f, %d links" % (every["ms"], len(every["a"])), flush=True)
quarter = 2
while quarter * 4 < max(first["n_links_all"], 8):
    quarter *= 2
os.environ["AGX_LINKS_SLOTS"] = str(quarter)
try:
    small = u.mate_links(w, 2)
    print("forced to %d slots: %d passes over the hits, ms %.3f; equal to the plain call: %s" % (quarter, small["n_passes"], small["ms"], LM.same(small, first) is None), flush=True)
except A.AgxError as x:
    print("forced to %d slots: refused (%s)" % (quarter, x.msg), flush=True)
del os.environ["AGX_LINKS_SLOTS"]
# the yardstick, for the kernel trace
u.pair_span()
print("for comparison: ms_pair_span %.3f (the whole unit)" % u.stats()["ms_pair_span"], flush=True)
print("device_bytes after every call %d; finish again gives the same bytes: %s" % (u.stats()["device_bytes"], u.finish() == fin), flush=True)
if not a.no_model:
    t_front, front = ms(u.front)
    f_lo, f_hi, at, kept, outside = SW.fragments_at({k: front[k] for k in ("n_pos", "dhit", "runs")})
    frags = (f_lo, f_hi, int(kept.sum()), int(outside.sum()))
    del front
    side = np.ascontiguousarray(u.walk_graph()["side_xpos"], np.uint32)
    t_ref, ref = ms(lambda: LM.mate_links(frags, st["n_pos"], side, w, 2))
    print("against links_model on %d fragments and %d side ids (front %.0f ms, model %.0f ms): first differing field %s; equal to the model: %s" %
          (len(f_lo), len(side), t_front, t_ref, LM.same(first, ref), LM.same(first, ref) is None), flush=True)
u.close()
