#!/usr/bin/env python3
"""What the evidence under the walk's records costs on a resident 30.4 Mb unit (the unit of the full-size export tests) after a finish, in one process:
  - agx_stats ms_walk_evidence of Unit.walk_evidence() at the run's coverage and support 2, without and with tracks, `rounds` times each after a warm-up (the first call
    also counts the edge support: reported apart), and once in forced chunks of 1 Mi bases;
  - the table's shape: graph bases, stretches, records, numbered steps, intervals, the longest record;
  - bytes the gather reads per base (a_nid 4, n_counts 24, n_next 16 + e_cnt 16 for a step, the stretch table's bisection apart) against the time of the call;
  - the same join through the host: Unit.graph() + Unit.edge_support() (wall time of each), then tests/evidence_model.py over the first records up to --model-bases
    graph bases, compared field by field with the device's tracks for those records.
Prints every value.  Not a test: nothing here asserts a time.
Usage (GPU box): python tests/tools/evidence_time.py [--work DIR]      (under rocprofv3 --kernel-trace --stats for agx_k_ev_gather and agx_k_ev_runs)"""
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
ap.add_argument("--work", default="/tmp/agx_evidence_time")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--model-bases", type=int, default=200000)
ap.add_argument("--no-host-path", action="store_true")
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
print("unit: %d positions, %d nodes, %d walk ids, %d overflow edges; hbm_needed %d; finish %.1f ms; device_bytes %d" %
      (st["n_pos"], st["n_nodes"], st["n_walk_ids"], st["n_edge_overflow"], need, t_fin, st["device_bytes"]), flush=True)
first = u.walk_evidence(w, 5, 2)
s1 = u.stats()
print("first call: ms_walk_evidence %.3f of which ms_edge_support %.3f (the counting); device_bytes %d" % (s1["ms_walk_evidence"], s1["ms_edge_support"], s1["device_bytes"]), flush=True)
print("table: %d records, %d stretches, %d graph bases (longest record %d), %d numbered steps, %d steps without an edge, %d intervals at depth 5 / support 2" %
      (len(w["rec_len"]), len(w["id_first"]), first["n_graph_bases"], int(first["rec_graph_bases"].max()) if len(w["rec_len"]) else 0, first["n_steps"],
       first["n_steps_without_edge"], len(first["iv_rec"])), flush=True)
plain, tracks, wall = [], [], []
for _ in range(a.rounds):
    t, _r = ms(lambda: u.walk_evidence(w, 5, 2))
    wall.append(t)
    plain.append(u.stats()["ms_walk_evidence"])
    u.walk_evidence(w, 5, 2, tracks=True)
    tracks.append(u.stats()["ms_walk_evidence"])
line("ms_walk_evidence, no tracks", plain)
line("ms_walk_evidence, tracks of every record", tracks)
line("Unit.walk_evidence(), no tracks, wall time of the Python call", wall)
os.environ["AGX_EVIDENCE_CHUNK"] = str(1 << 20)
chunked = u.walk_evidence(w, 5, 2)
print("in chunks of 1 Mi bases: ms_walk_evidence %.3f" % u.stats()["ms_walk_evidence"], flush=True)
del os.environ["AGX_EVIDENCE_CHUNK"]
import evidence_model as EM   # noqa: E402
print("chunked answer equals the unchunked one:", EM.same(chunked, first) is None, flush=True)
n = max(int(first["n_graph_bases"]), 1)
per_base = 4 + 24 + 32.0 * first["n_steps"] / n
print("gathered bytes per base %.1f (of %d bases: %.1f MB); at min ms_walk_evidence that is %.1f GB/s for the whole call" %
      (per_base, n, per_base * n / 1e6, per_base * n / 1e6 / max(min(plain), 1e-9)), flush=True)
print("device_bytes after every call %d; finish again gives the same bytes: %s" % (u.stats()["device_bytes"], u.finish() == fin), flush=True)
if not a.no_host_path:
    t_g, g = ms(u.graph)
    t_s, sup = ms(u.edge_support)
    print("host path: Unit.graph() %.1f ms, Unit.edge_support() %.1f ms" % (t_g, t_s), flush=True)
    import walk_model as WM   # noqa: E402
    gb = np.cumsum(first["rec_graph_bases"].astype(np.int64))
    hi = int(np.searchsorted(gb, a.model_bases, side="right"))
    hi = max(1, min(hi, len(w["rec_len"])))
    so = w["st_off"].astype(np.int64)
    sub = {"rec_len": w["rec_len"][:hi], "st_off": w["st_off"][:hi + 1], "id_first": w["id_first"][:so[hi]], "id_last": w["id_last"][:so[hi]],
           "base_off": w["base_off"][:so[hi]], "joined": w["joined"][:so[hi]]}
    g.update({"pos_nuc": b"N" * int(g["n_pos"]), "chain_end": np.zeros(g["n_pos"], np.uint32), "cm_count": np.zeros(g["n_pos"], np.uint32), "hop_off": np.zeros(g["n_pos"], np.uint32),
              "hop_len": np.zeros(g["n_pos"], np.uint32), "hop_end": np.zeros(g["n_pos"], np.uint32), "hop_str": b""})
    t_m, want = ms(lambda: EM.evidence(g, 5, sub, sup, 5, 2, wm=WM.build(g, 5)))
    got = u.walk_evidence(sub, 5, 2, tracks=True)
    print("model over the first %d records (%d graph bases): %.1f ms; equal to the device's answer for them: %s" % (hi, int(want["n_graph_bases"]), t_m, EM.same(got, want, tracks=True) is None), flush=True)
u.close()
