#!/usr/bin/env python3
"""What edge support costs on a resident 30.4 Mb unit (the unit of the full-size export tests), in one process:
  - the counting: agx_stats ms_edge_support of the first export with support after each of `rounds` builds of the resident unit (a 1 000-position window, so that the
    call is the counting and little else), and of a second call (the counters are reused);
  - agx_unit_edge_support: wall time of the whole call (the counting is done: the rest is the copies and the host's renumbering);
  - agx_unit_unitigs_support against agx_unit_unitigs_region for the whole window and for a 100 000-position window in the middle: a warm-up of each, then `rounds`
    alternations, wall times of the Python calls.
Prints every value.  Not a test: nothing here asserts a time.
Usage (GPU box): python tests/tools/edge_support_time.py [--work DIR]      (under rocprofv3 --kernel-trace --stats for agx_k_edge_support beside agx_k_node_sweep<0>)"""
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
ap.add_argument("--work", default="/tmp/agx_edge_support_time")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()

run = H.synth(a.work, seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
tmp = os.path.join(run, "tmp")
A.cache_build(tmp, 0)


def ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def line(name, v):
    print("%-78s min %10.3f ms   all %s" % (name, min(v), " ".join("%.3f" % x for x in v)), flush=True)


plain = A.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True)
plain.load_files(tmp, 0)
need_plain = plain.hbm_needed()
plain.close()
u = A.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True, edge_support=True)
u.load_files(tmp, 0)
need = u.hbm_needed()
u.upload()
u.build()
st = u.stats()
n_pos = st["n_pos"]
print("unit: %d positions, %d nodes, %d tile entries, %d overflow edges, from_cache %d; hbm_needed %d with the flag, %d without (+%d)" %
      (n_pos, st["n_nodes"], st["n_tile_entries"], st["n_edge_overflow"], st["from_cache"], need, need_plain, need - need_plain), flush=True)
small = (n_pos // 2, n_pos // 2 + 1000)
count, again = [], []
for _ in range(a.rounds):
    u.build()
    u.unitigs(region=small, edge_support=True)
    count.append(u.stats()["ms_edge_support"])
    u.unitigs(region=small, edge_support=True)
    again.append(u.stats()["ms_edge_support"])
line("ms_edge_support, first call after a build (zero, agx_k_edge_support, totals)", count)
line("ms_edge_support, second call (counters reused)", again)
print("events %d" % u.stats()["n_support_events"], flush=True)
whole_call = [ms(u.edge_support) for _ in range(2)]
line("agx_unit_edge_support, counters valid (copies + renumbering on the host)", whole_call)
s = u.edge_support()
print("edges %d, contributions %d, events %d, largest support %d, edges with support 1: %d" %
      (s["n_edges"], s["n_contributions"], s["n_events"], int(s["edge_cnt"].max()), int((s["edge_cnt"] == 1).sum())), flush=True)
mid = (n_pos // 2 - 50000, n_pos // 2 + 50000)
for name, region in (("whole window", (0, n_pos)), ("100 000-position window", mid)):
    u.unitigs(region=region, edge_support=True)
    u.unitigs(region=region)
    with_sup, without = [], []
    for _ in range(a.rounds):
        with_sup.append(ms(lambda: u.unitigs(region=region, edge_support=True)))
        without.append(ms(lambda: u.unitigs(region=region)))
    line("Unit.unitigs(edge_support=True), %s" % name, with_sup)
    line("Unit.unitigs(), region form, %s" % name, without)
t = u.unitigs(region=mid, edge_support=True)
print("100 000-position window: %d segments, %d links, link support min %d max %d" %
      (len(t["head_pos"]), len(t["link_from"]), int(t["link_support"].min()) if len(t["link_support"]) else 0, int(t["link_support"].max()) if len(t["link_support"]) else 0))
u.close()
