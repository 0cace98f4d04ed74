"""Hand-made fronts for the pair-span tests (tests/test_span_model.py, tests/test_span_cases.py): derived hit records and runs in the layout of Unit.front() /
hostsim's front, written hit by hit, so that a test can say exactly where every mate lies.  Nothing here is a unit the engine can load: the GPU tests take their
fronts from real units."""
import numpy as np

import aligngraph_amd as A

HF_SKIP = 2
DHIT = np.dtype(A.FRONT_DHIT)
RUN = np.dtype(A.FRONT_RUN)
assert DHIT.itemsize == 40 and RUN.itemsize == 12


def hand_front(n_pos, hits):
    """hits: dicts with a, b — a mate's reference offset of read index 0 (a simple mate) or its runs [(q, t, n), ...] —, len, and optionally skip=True.
    Returns {"n_pos", "dhit", "runs"}.  Where both mates are simple a_runs / b_runs hold what hit_prep leaves there (no run indexes), to show that nobody reads them so."""
    runs = [(0, 0, 0)]                                 # (run 0 belongs to nobody: an index of 0 is a real index for the hits below)
    d = np.zeros(len(hits), DHIT)
    for i, h in enumerate(hits):
        d[i]["len"], d[i]["flags"], d[i]["jstar"] = h["len"], HF_SKIP if h.get("skip") else 0, 0xFFFF
        for m in "ab":
            if isinstance(h[m], int):
                d[i][m + "_t0"] = h[m]
            else:
                d[i][m + "_runs"], d[i][m + "_nruns"] = len(runs), len(h[m])
                runs.extend(h[m])
        if isinstance(h["a"], int) and isinstance(h["b"], int):
            d[i]["a_runs"], d[i]["b_runs"] = 0xFFF00000 | h["len"], 0
    return {"n_pos": n_pos, "dhit": d, "runs": np.array(runs, RUN)}


def window_fronts(n_pos=200):
    """name -> front: the shapes a window's borders can cut (the windows of tests/test_span_cases.py are cut around positions 63 .. 65 and 100 .. 140)."""
    return {
        "b_left_of_a": hand_front(n_pos, [dict(a=120, b=40, len=20), dict(a=60, b=62, len=10)]),
        "one_inside_the_other": hand_front(n_pos, [dict(a=[(0, 50, 30), (30, 90, 30)], b=70, len=60), dict(a=64, b=64, len=1)]),
        "skipped": hand_front(n_pos, [dict(a=10, b=100, len=30, skip=True), dict(a=63, b=65, len=2)]),
        "covers_the_window": hand_front(n_pos, [dict(a=0, b=170, len=30), dict(a=101, b=130, len=5)]),
        "left_border_only": hand_front(n_pos, [dict(a=40, b=60, len=10)]),          # [40, 69]: across 63 / 64, not across 100 or 140
        "right_border_only": hand_front(n_pos, [dict(a=120, b=150, len=10)]),       # [120, 159]: across 139 / 140
        "over_the_end": hand_front(n_pos, [dict(a=150, b=195, len=20), dict(a=200, b=230, len=20), dict(a=199, b=199, len=1)]),
        "nothing": hand_front(n_pos, []),
    }
