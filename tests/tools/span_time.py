#!/usr/bin/env python3
"""What the pair span costs on a resident 30.4 Mb unit (the unit of the full-size export tests) at coverage 5 after a finish, in one process:
  - agx_stats ms_pair_span of Unit.pair_span() for the whole unit and for a window of 100 000 positions, `rounds` times each after a warm-up, and once in forced
    sub-windows of 4 Mi positions (each one more pass over the hits);
  - agx_stats ms_walk_span of Unit.walk_span() on the table of the unit's own finish at min_span 2, without and with tracks, and once in forced chunks of 1 Mi bases;
  - the shapes: hits, kept hits, fragments, the largest span; records, stretches, graph bases, numbered steps, jump steps, steps not forward, thin intervals;
  - for comparison in the same trace, one Unit.edge_support() (agx_k_edge_support) and one Unit.walk_evidence() (agx_k_ev_gather) — the unit is created with edge_support
    for that alone: the pair span does not need it;
  - the whole unit's span, cross and counts against tests/span_wide.py (sorted endpoints, fast at this size) on the front Unit.front() copies out: a reference, where the
    model's loops are for the small units of the tests;
  - consistency: cross <= span, cross at the last position is 0, a window equals the whole unit's slice, forced sub-windows and forced base chunks equal the plain calls.
Prints every value.  Not a test: nothing here asserts a time.
Usage (GPU box): python tests/tools/span_time.py [--work DIR]      (under rocprofv3 --kernel-trace --stats for the kernels of agx_span.hip)"""
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
import span_model as SM      # noqa: E402
import span_wide as SW       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--work", default="/tmp/agx_span_time")
ap.add_argument("--rounds", type=int, default=3)
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


u = A.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True, keep_paths=True, edge_support=True)
u.load_files(tmp, 0)
need = u.hbm_needed()
u.upload()
u.build()
t_fin, fin = ms(u.finish)
w = u.walk_paths()
st = u.stats()
n_pos = st["n_pos"]
print("unit: %d positions, %d hits, %d runs, %d nodes, %d walk ids; hbm_needed %d; finish %.1f ms; device_bytes %d" %
      (n_pos, st["n_hits"], st["n_runs"], st["n_nodes"], st["n_walk_ids"], need, t_fin, st["device_bytes"]), flush=True)
first = u.pair_span()
s1 = u.stats()
print("first call: ms_pair_span %.3f; device_bytes %d" % (s1["ms_pair_span"], s1["device_bytes"]), flush=True)
print("pair span: %d kept hits, %d fragments, %d outside; largest span %d, mean span %.2f; cross <= span everywhere: %s; cross at the last position %d" %
      (first["n_kept"], first["n_fragments"], first["n_outside"], int(first["span"].max()), float(first["span"].mean()), bool((first["cross"] <= first["span"]).all()), int(first["cross"][-1])), flush=True)
t_front, front = ms(u.front)
t_ref, ref = ms(lambda: SW.pair_span({k: front[k] for k in ("n_pos", "dhit", "runs")}))
print("the whole unit against span_wide on the front of %d hit records and %d runs (front %.0f ms, reference %.0f ms): first differing field %s; equal to the wide reference: %s" %
      (len(front["dhit"]), len(front["runs"]), t_front, t_ref, SM.same_span(first, ref), SM.same_span(first, ref) is None), flush=True)
del front
whole, window, wall = [], [], []
mid = (n_pos // 2, n_pos // 2 + 100000)
for _ in range(a.rounds):
    t, _r = ms(u.pair_span)
    wall.append(t)
    whole.append(u.stats()["ms_pair_span"])
    u.pair_span(mid)
    window.append(u.stats()["ms_pair_span"])
line("ms_pair_span, the whole unit", whole)
line("ms_pair_span, a window of 100 000 positions", window)
line("Unit.pair_span(), the whole unit, wall time of the Python call", wall)
os.environ["AGX_SPAN_CHUNK"] = str(4 << 20)
sub = u.pair_span()
print("in sub-windows of 4 Mi positions (%d passes over the hits): ms_pair_span %.3f; equal to the plain call: %s" %
      (-(-n_pos // (4 << 20)), u.stats()["ms_pair_span"], SM.same_span(sub, first) is None), flush=True)
del os.environ["AGX_SPAN_CHUNK"]
got_mid = u.pair_span(mid)
print("the window equals the whole unit's slice: %s" % (np.array_equal(got_mid["span"], first["span"][mid[0]:mid[1]]) and np.array_equal(got_mid["cross"], first["cross"][mid[0]:mid[1]])), flush=True)
e0 = u.walk_span(w, 2)
s2 = u.stats()
print("first walk_span: ms_walk_span %.3f; device_bytes %d" % (s2["ms_walk_span"], s2["device_bytes"]), flush=True)
print("table: %d records, %d stretches, %d graph bases (longest record %d), %d numbered steps, %d jump steps, %d steps not forward, %d thin intervals at min_span 2" %
      (len(w["rec_len"]), len(w["id_first"]), e0["n_graph_bases"], int(e0["rec_graph_bases"].max()) if len(w["rec_len"]) else 0, e0["n_steps"], e0["n_jump_steps"],
       e0["n_steps_not_forward"], len(e0["iv_rec"])), flush=True)
plain, tracks = [], []
for _ in range(a.rounds):
    u.walk_span(w, 2)
    plain.append(u.stats()["ms_walk_span"])
    u.walk_span(w, 2, tracks=True)
    tracks.append(u.stats()["ms_walk_span"])
line("ms_walk_span, no tracks", plain)
line("ms_walk_span, tracks of every record", tracks)
os.environ["AGX_SPAN_BASE_CHUNK"] = str(1 << 20)
chunked = u.walk_span(w, 2)
print("in chunks of 1 Mi bases: ms_walk_span %.3f; equal to the plain call: %s" % (u.stats()["ms_walk_span"], SM.same(chunked, e0) is None), flush=True)
del os.environ["AGX_SPAN_BASE_CHUNK"]
# the two yardsticks, for the kernel trace
t_s, sup = ms(u.edge_support)
u.walk_evidence(w, 5, 2)
s3 = u.stats()
print("for comparison: Unit.edge_support() %.1f ms (ms_edge_support %.3f, %d events), ms_walk_evidence %.3f" % (t_s, s3["ms_edge_support"], s3["n_support_events"], s3["ms_walk_evidence"]), flush=True)
print("device_bytes after every call %d; finish again gives the same bytes: %s" % (u.stats()["device_bytes"], u.finish() == fin), flush=True)
u.close()
