#!/usr/bin/env python3
"""What edge reads cost on a resident 30.4 Mb unit (the unit of the full-size export tests), in one process:
  - the counting first (agx_unit_edge_support's first call after each build), so that the same trace holds agx_k_edge_support beside the two passes of agx_k_edge_reads;
  - Unit.edge_reads() of the whole unit at max_support 1 and 2 and of a 100 000-position window in the middle at both: agx_stats ms_edge_reads and the wall time of the
    Python call per round, the edges and records that came back and the bytes of records copied out (16 per record);
  - one forced-chunk run of the whole unit at max_support 2 (AGX_EDGE_READS_CHUNK), which must give the same table; with AGX_TRACE=1 the library prints the chunk count
    of every call on stderr;
  - hbm_needed and device_bytes before and after.
Prints every value.  Not a test: nothing here asserts a time.  The whole unit at 0xFFFFFFFF (hundreds of millions of records) is not asked for.
Usage (GPU box): python tests/tools/edge_reads_time.py [--work DIR] [--rounds N] [--chunk TILES]
                 (under rocprofv3 --kernel-trace --stats for agx_k_edge_reads<false> / <true> beside agx_k_edge_support)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import harness as H          # noqa: E402
import aligngraph_amd as A   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--work", default="/tmp/agx_edge_support_time")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--chunk", type=int, default=65536)
a = ap.parse_args()

run = H.synth(a.work, seed=1000, chroms="30427671", pairs=3000000, L=100, k=5, coverage=5, sam_seq=0, threads=16)
tmp = os.path.join(run, "tmp")
A.cache_build(tmp, 0)


def line(name, v):
    print("%-86s min %10.3f ms   all %s" % (name, min(v), " ".join("%.3f" % x for x in v)), flush=True)


u = A.Unit(k=5, insert_variation=50, coverage=5, keep_counts=True, edge_support=True)
u.load_files(tmp, 0)
need = u.hbm_needed()
u.upload()
u.build()
st = u.stats()
n_pos, dev0 = st["n_pos"], st["device_bytes"]
print("unit: %d positions, %d nodes, %d tiles, %d tile entries, %d overflow edges; hbm_needed %d, device_bytes %d" %
      (n_pos, st["n_nodes"], st["n_tiles"], st["n_tile_entries"], st["n_edge_overflow"], need, dev0), flush=True)
count = []
for _ in range(a.rounds):
    u.build()
    s = u.edge_support()
    count.append(u.stats()["ms_edge_support"])
line("ms_edge_support, first call after a build (zero, agx_k_edge_support, totals)", count)
print("edges %d, contributions %d, events %d, edges with support 1: %d, with support 2: %d" %
      (s["n_edges"], s["n_contributions"], s["n_events"], int((s["edge_cnt"] == 1).sum()), int((s["edge_cnt"] == 2).sum())), flush=True)
mid = (n_pos // 2 - 50000, n_pos // 2 + 50000)
answers = {}
for name, region in (("whole unit", None), ("100 000-position window", mid)):
    for top in (1, 2):
        u.edge_reads(region, top)      # warm-up
        inside, wall = [], []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            r = u.edge_reads(region, top)
            wall.append((time.perf_counter() - t0) * 1e3)
            inside.append(u.stats()["ms_edge_reads"])
        answers[(name, top)] = r
        line("ms_edge_reads, %s, max_support %d" % (name, top), inside)
        line("Unit.edge_reads() wall, %s, max_support %d" % (name, top), wall)
        print("    %d edges, %d records, %d bytes of records copied out, supports %s" %
              (len(r["src_pos"]), len(r["hit"]), 16 * len(r["hit"]), np.bincount(r["support"].astype(np.int64)).tolist()), flush=True)
os.environ["AGX_EDGE_READS_CHUNK"] = str(a.chunk)
t0 = time.perf_counter()
forced = u.edge_reads(None, 2)
wall = (time.perf_counter() - t0) * 1e3
del os.environ["AGX_EDGE_READS_CHUNK"]
want = answers[("whole unit", 2)]
print("forced chunks of %d tiles (%d chunks): ms_edge_reads %.3f, wall %.3f ms, equal to the unforced answer: %s" %
      (a.chunk, (st["n_tiles"] + a.chunk - 1) // a.chunk, u.stats()["ms_edge_reads"], wall, all(np.array_equal(forced[k], want[k]) for k in want)), flush=True)
print("hbm_needed %d (before: %d), device_bytes %d (before: %d)" % (u.hbm_needed(), need, u.stats()["device_bytes"], dev0), flush=True)
u.close()
