#!/usr/bin/env python3
"""What the bubbles cost on a resident 30.4 Mb unit (the unit of the full-size export tests) at coverage 5, in one process:
  - the call's own time (agx_bubbles.ms) of Unit.bubbles() over every position at the unit's coverage, `rounds` times after a warm-up, with the wall time of the Python
    call and the bytes it brought down;
  - the yardstick, the only way to the same answer without the call: Unit.unitigs(region, min_coverage) over the same window plus unitigs_bubbles() on its table —
    the wall time of each, alternating with the call, and the bytes the export brought down;
  - once with support (agx_k_utr_link_support and agx_k_bb_support in the trace), and at min_coverage 0;
  - the unit's totals: forks by class, the k histogram, the longest branch, direct against segment branches;
  - consistency: the call equals the twin on the export (with support too), device_bytes and hbm_needed() before and after, a finish behind it all.
Prints every value.  Not a test: nothing here asserts a time.
Usage (GPU box): python tests/tools/bubbles_time.py [--work DIR] [--rounds N]      (under rocprofv3 --kernel-trace --stats for the kernels of agx_bubbles.hip beside
agx_k_utr_link_support and phase 3's agx_k_utr_emit / agx_k_ut_links_sort)"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--work", default="/tmp/agx_bubbles_time")
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

run = H.synth(a.work, seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
tmp = os.path.join(run, "tmp")
A.cache_build(tmp, 0)
FIELDS = ("n_segs", "n_links", "n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared", "longest_branch",
          "src_pos", "src_var", "src_last", "sink_pos", "sink_var", "br_off", "br_pos", "br_var", "br_nodes", "br_cov", "br_seq_off")


def ms(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def line(name, v):
    print("%-86s min %10.3f ms   all %s" % (name, min(v), " ".join("%.3f" % x for x in v)), flush=True)


def same(x, y):
    return all(np.array_equal(x[f], y[f]) for f in FIELDS + (("br_sup_in", "br_sup_out") if x["has_support"] else ())) and bytes(x["seq"]) == bytes(y["seq"]) and x["has_support"] == y["has_support"]


print("library: %s" % A.LIB_PATH, flush=True)
u = A.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True, edge_support=True)
u.load_files(tmp, 0)
need = u.hbm_needed()
u.upload()
u.build()
st = u.stats()
n = st["n_pos"]
print("unit: %d positions, %d hits, %d nodes; hbm_needed %d; device_bytes %d" % (n, st["n_hits"], st["n_nodes"], need, st["device_bytes"]), flush=True)
t0 = u.unitigs(region=(0, n), min_coverage=5)
held = u.stats()["device_bytes"]
ns, nl, nb = len(t0["head_pos"]), len(t0["link_from"]), len(t0["seq"])
export_bytes = ns * (4 * 4 + 8) + 2 * 4 * (ns + 1) + 4 * nl + nb
first = u.bubbles(region=(0, n), min_coverage=5)
print("first call: ms %.3f; device_bytes %d (after the first export %d)" % (first["ms"], u.stats()["device_bytes"], held), flush=True)
call, wall, exp, twin = [], [], [], []
for _ in range(a.rounds):
    t, b = ms(lambda: u.bubbles(region=(0, n), min_coverage=5))
    wall.append(t)
    call.append(b["ms"])
    t, tab = ms(lambda: u.unitigs(region=(0, n), min_coverage=5))
    exp.append(t)
    t, tw = ms(lambda: A.unitigs_bubbles(tab))
    twin.append(t)
line("agx_bubbles.ms, every position at coverage 5", call)
line("Unit.bubbles(), wall time of the Python call", wall)
line("the yardstick: Unit.unitigs(region, min_coverage), wall time of the Python call", exp)
line("the yardstick: unitigs_bubbles() on its table, wall time of the Python call", twin)
line("the yardstick, both", [x + y for x, y in zip(exp, twin)])
print("bytes brought down: the call %d, the export %d (%d segments, %d links, %d bases)" % (b["bytes_down"], export_bytes, ns, nl, nb), flush=True)
print("the call equals the twin on the export: %s" % same(b, tw), flush=True)
k = np.diff(b["br_off"].astype(np.int64))
direct = np.add.reduceat((b["br_pos"] == 0xFFFFFFFF).astype(np.int64), b["br_off"][:-1].astype(np.int64)) if len(k) else np.zeros(0, np.int64)
print("totals at coverage 5: %d segments, %d links, %d forks = %d bubbles + %d TIP + %d NESTED + %d SINKS_DIFFER + %d SINK_SHARED; longest branch %d nodes" %
      tuple(int(b[f]) for f in FIELDS[:9]), flush=True)
print("k histogram of the bubbles: %s; bubbles with a direct branch %d, with segment branches only %d; branch rows %d, bases %d" %
      (" ".join("%d:%d" % (v, c) for v, c in zip(*np.unique(k, return_counts=True))), int((direct > 0).sum()), int((direct == 0).sum()), len(b["br_pos"]), len(b["seq"])), flush=True)
nodes = b["br_nodes"][b["br_pos"] != 0xFFFFFFFF]
print("nodes of the branch segments: %s" % " ".join("%s:%d" % (lab, int(((nodes >= lo) & (nodes < hi)).sum())) for lab, lo, hi in
                                                     (("1", 1, 2), ("2-3", 2, 4), ("4-7", 4, 8), ("8-15", 8, 16), ("16-63", 16, 64), ("64+", 64, 1 << 32))), flush=True)
ts, bs = ms(lambda: u.bubbles(region=(0, n), min_coverage=5, edge_support=True))
counting = u.stats()["ms_edge_support"]
tabs = u.unitigs(region=(0, n), min_coverage=5, edge_support=True)
print("with support: first call %.3f ms wall (makes the counters: ms_edge_support %.3f); equal to the twin on the export with support: %s" %
      (ts, counting, same(bs, A.unitigs_bubbles(tabs, tabs["link_support"]))), flush=True)
sup = [u.bubbles(region=(0, n), min_coverage=5, edge_support=True)["ms"] for _ in range(a.rounds)]
line("agx_bubbles.ms with support", sup)
b0 = u.bubbles(region=(0, n), min_coverage=0)
print("at min_coverage 0: ms %.3f; %d segments, %d links, %d forks = %d bubbles + %d TIP + %d NESTED + %d SINKS_DIFFER + %d SINK_SHARED; longest branch %d nodes" %
      ((b0["ms"],) + tuple(int(b0[f]) for f in FIELDS[:9])), flush=True)
small = [u.bubbles(region=(n // 2, n // 2 + 100000), min_coverage=5)["ms"] for _ in range(a.rounds)]
line("agx_bubbles.ms, a window of 100 000 positions", small)
print("device_bytes after every call %d (with support the per-link array of the export); hbm_needed %d" % (u.stats()["device_bytes"], u.hbm_needed()), flush=True)
fin = u.finish()
again = u.bubbles(region=(0, n), min_coverage=5)
print("behind a finish: ms %.3f, equal to the first call: %s; a second finish gives the same bytes: %s" % (again["ms"], same(again, first), u.finish() == fin), flush=True)
u.close()
