"""Plain-Python model of the bubbles (agx_unit_bubbles / agx_unitigs_bubbles).  It imports nothing of the project and shares nothing with the kernels.

The graph is a unitig table shaped like tests/unitig_region_model.py's (head_pos, head_var, n_nodes, last_pos, coverage, seq_off, seq, link_from, link_to; arrays or
lists), with the links' support as an optional list.  out(s) are the links that leave s in the table's order, in(s) the number that enter it.

  fork          a segment S with k = |out(S)| >= 2
  branch        a target X with in(X) == 1 is a branch SEGMENT, its exit the target of its one link when |out(X)| == 1;
                a target with in(X) >= 2 is a DIRECT branch, its exit X itself
  class         the first that applies: TIP (a branch segment without a link), NESTED (one with two links or more), SINKS_DIFFER (the exits are not one segment),
                SINK_SHARED (in of the common exit T > k), BUBBLE with sink T

bubbles() returns what Unit.bubbles() returns, as plain ints, lists and bytes: the totals, and the table of the bubbles whose branch segments have max_nodes nodes at
most.  classes() returns the class of every fork, for the tests that want to know which fork is which.
"""
NONE = 0xFFFFFFFF
TOTALS = ("n_segs", "n_links", "n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared", "longest_branch")
PER_BUBBLE = ("src_pos", "src_var", "src_last", "sink_pos", "sink_var", "br_off")
PER_BRANCH = ("br_pos", "br_var", "br_nodes", "br_cov", "br_seq_off")
SUPPORT = ("br_sup_in", "br_sup_out")


def _ints(a):
    return [int(v) for v in a]


def adjacency(t):
    """(out, n_in): per segment the list of (link number, target) in the table's order, and the number of links that enter it"""
    n = len(t["head_pos"])
    out, n_in = [[] for _ in range(n)], [0] * n
    for i, (a, b) in enumerate(zip(_ints(t["link_from"]), _ints(t["link_to"]))):
        out[a].append((i, b))
        n_in[b] += 1
    return out, n_in


def classify(s, out, n_in):
    """('none' | 'tip' | 'nested' | 'sinks_differ' | 'sink_shared' | 'bubble', sink or None) of segment s"""
    k = len(out[s])
    if k < 2:
        return "none", None
    segs = [x for _, x in out[s] if n_in[x] == 1]
    if any(len(out[x]) == 0 for x in segs):
        return "tip", None
    if any(len(out[x]) >= 2 for x in segs):
        return "nested", None
    exits = {out[x][0][1] if n_in[x] == 1 else x for _, x in out[s]}
    if len(exits) != 1:
        return "sinks_differ", None
    sink = exits.pop()
    assert n_in[sink] >= k, "k distinct links enter the sink"
    return ("sink_shared", None) if n_in[sink] > k else ("bubble", sink)


def classes(t):
    """{segment: (class, sink)} of every fork"""
    out, n_in = adjacency(t)
    got = {s: classify(s, out, n_in) for s in range(len(out))}
    return {s: c for s, c in got.items() if c[0] != "none"}


def bubbles(t, link_support=None, max_nodes=None):
    out, n_in = adjacency(t)
    hp, hv, nn, lp, cov, so = (_ints(t[f]) for f in ("head_pos", "head_var", "n_nodes", "last_pos", "coverage", "seq_off"))
    seq = bytes(t["seq"])
    sup = _ints(link_support) if link_support is not None else None
    b = {f: 0 for f in TOTALS}
    b.update({f: [] for f in PER_BUBBLE + PER_BRANCH})
    b.update(n_segs=len(hp), n_links=len(_ints(t["link_from"])), seq=b"", has_support=sup is not None)
    if sup is not None:
        b.update({f: [] for f in SUPPORT})
    for s in range(len(hp)):
        cls, sink = classify(s, out, n_in)
        if cls == "none":
            continue
        b["n_forks"] += 1
        b[{"bubble": "n_bubbles_all", "tip": "n_tip", "nested": "n_nested", "sinks_differ": "n_sinks_differ", "sink_shared": "n_sink_shared"}[cls]] += 1
        if cls != "bubble":
            continue
        longest = max([nn[x] for _, x in out[s] if n_in[x] == 1], default=0)
        b["longest_branch"] = max(b["longest_branch"], longest)
        if max_nodes is not None and longest > max_nodes:
            continue
        assert sum(1 for _, x in out[s] if n_in[x] >= 2) <= 1, "a bubble has one direct branch at most"
        b["src_pos"].append(hp[s]); b["src_var"].append(hv[s]); b["src_last"].append(lp[s]); b["sink_pos"].append(hp[sink]); b["sink_var"].append(hv[sink])
        b["br_off"].append(len(b["br_pos"]))
        for i, x in out[s]:
            b["br_seq_off"].append(len(b["seq"]))
            if n_in[x] == 1:
                j = out[x][0][0]
                b["br_pos"].append(hp[x]); b["br_var"].append(hv[x]); b["br_nodes"].append(nn[x]); b["br_cov"].append(cov[x])
                b["seq"] += seq[so[x]:so[x] + nn[x]]
            else:
                j = i
                b["br_pos"].append(NONE); b["br_var"].append(NONE); b["br_nodes"].append(0); b["br_cov"].append(0)
            if sup is not None:
                b["br_sup_in"].append(sup[i]); b["br_sup_out"].append(sup[j])
    b["br_off"].append(len(b["br_pos"]))
    b["br_seq_off"].append(len(b["seq"]))
    assert b["n_forks"] == b["n_bubbles_all"] + b["n_tip"] + b["n_nested"] + b["n_sinks_differ"] + b["n_sink_shared"]
    return b


def mismatch(got, want):
    """First difference between a table of the library's (numpy arrays) and the model's, as text, or None."""
    for f in TOTALS:
        if int(got[f]) != want[f]:
            return "%s = %d, expected %d" % (f, int(got[f]), want[f])
    if bool(got["has_support"]) != want["has_support"]:
        return "has_support = %s" % got["has_support"]
    for f in PER_BUBBLE + PER_BRANCH + (SUPPORT if want["has_support"] else ()):
        a, w = _ints(got[f]), want[f]
        i = next((i for i in range(min(len(a), len(w))) if a[i] != w[i]), None)
        if i is not None:
            return "%s[%d] = %d, expected %d" % (f, i, a[i], w[i])
        if len(a) != len(w):
            return "%s has %d entries, expected %d" % (f, len(a), len(w))
    if bytes(got["seq"]) != want["seq"]:
        return "seq differs (%d bytes, expected %d)" % (len(got["seq"]), len(want["seq"]))
    return None


def tsv(b, unit=0):
    """The text of agx_bubbles_tsv, from a table of the model's or the library's."""
    def name(p, v):
        return "*" if int(p) == NONE and int(v) == NONE else "u%d_%d_%d" % (unit, int(p), int(v))
    seq, lines = bytes(b["seq"]).decode(), []
    so = _ints(b["br_seq_off"])
    for i in range(len(b["src_pos"])):
        rows = range(int(b["br_off"][i]), int(b["br_off"][i + 1]))
        direct = [int(b["br_pos"][r]) == NONE and int(b["br_var"][r]) == NONE for r in rows]
        sups = [",".join(str(int(b[f][r])) for r in rows) for f in SUPPORT] if b["has_support"] else [".", "."]
        lines.append("\t".join([name(b["src_pos"][i], b["src_var"][i]), name(b["sink_pos"][i], b["sink_var"][i]), str(int(b["src_last"][i])), str(int(b["sink_pos"][i])), str(len(rows)),
                                ",".join(name(b["br_pos"][r], b["br_var"][r]) for r in rows), ",".join(str(int(b["br_nodes"][r])) for r in rows),
                                ",".join(str(int(b["br_cov"][r])) for r in rows)] + sups +
                               [",".join("*" if d else seq[so[r]:so[r + 1]] for r, d in zip(rows, direct))]))
    return ("".join(l + "\n" for l in lines)).encode()
