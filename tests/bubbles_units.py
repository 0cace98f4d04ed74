"""Hand-made tables and units that pin the bubbles (agx_unit_bubbles / agx_unitigs_bubbles, agx_bubbles.hip).

hand_table() is a written-out unitig table with its expected answer beside it: one fork of each class, a three-way bubble with a direct branch, a bubble whose sink is
the next bubble's source.  The units are lean_units.Unit's written by walk_units.write_unit, so the CPU file (tests/test_bubbles_cases.py) and the GPU file
(tests/test_gpu_bubbles.py) build the same inputs; what is correct is decided by tests/bubbles_model.py on the region model's table of the oracle's graph.  Each unit
names its windows (lo, hi, threshold) and what the model must show there (`want`: predicates on the model's answer), so a unit cannot silently stop making its shape.
"""
import edge_units as EU
from edge_units import cover, dele
from lean_units import Unit

NONE = 0xFFFFFFFF


# ---- the hand table ------------------------------------------------------------------------------------------------------------------------
#   0 -> 1, 2, 3; 1 -> 3; 2 -> 3          a three-way BUBBLE 0 => 3: two segment branches (2 and 5 nodes) and a direct one
#   3 -> 4, 5; 4 -> 6; 5 -> 6             a BUBBLE 3 => 6 whose source is the first one's sink: two segment branches of one node
#   7 -> 8, 9; 9 -> 10                    TIP: 8 has no link
#   11 -> 12, 13; 12 -> 14, 15; 13 -> 15  NESTED at 11 (12 has two links); 12 itself is a TIP (14 has no link)
#   16 -> 17, 18; 17 -> 19; 18 -> 20      SINKS_DIFFER
#   21 -> 22, 23; 22 -> 24; 23 -> 24; 25 -> 24      SINK_SHARED: three links enter 24
HAND_LINKS = [(0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (3, 4), (3, 5), (4, 6), (5, 6), (7, 8), (7, 9), (9, 10), (11, 12), (11, 13), (12, 14), (12, 15), (13, 15),
              (16, 17), (16, 18), (17, 19), (18, 20), (21, 22), (21, 23), (22, 24), (23, 24), (25, 24)]
HAND_NODES = [3, 2, 5, 4, 1, 1, 2, 1, 2, 3, 1, 2, 1, 3, 1, 2, 2, 1, 1, 3, 1, 2, 2, 2, 1, 4]
HAND_LONGEST = 5


def hand_table():
    """(table, link_support): 26 segments; segment s heads position 100 s as variant s % 2, its bases are the letters "ACGT"[(s + j) % 4], its coverage 10 s + 1"""
    n = len(HAND_NODES)
    off = [sum(HAND_NODES[:s]) for s in range(n + 1)]
    t = {"head_pos": [100 * s for s in range(n)], "head_var": [s % 2 for s in range(n)], "n_nodes": list(HAND_NODES), "last_pos": [100 * s + HAND_NODES[s] - 1 for s in range(n)],
         "coverage": [10 * s + 1 for s in range(n)], "seq_off": off, "seq": "".join("ACGT"[(s + j) % 4] for s in range(n) for j in range(HAND_NODES[s])).encode(),
         "link_from": [a for a, _ in HAND_LINKS], "link_to": [b for _, b in HAND_LINKS]}
    return t, [1000 + i for i in range(len(HAND_LINKS))]


HAND_TOTALS = {"n_segs": 26, "n_links": 26, "n_forks": 7, "n_bubbles_all": 2, "n_tip": 2, "n_nested": 1, "n_sinks_differ": 1, "n_sink_shared": 1, "longest_branch": 5}
HAND_CLASSES = {0: ("bubble", 3), 3: ("bubble", 6), 7: ("tip", None), 11: ("nested", None), 12: ("tip", None), 16: ("sinks_differ", None), 21: ("sink_shared", None)}
# the table with every bubble (max_nodes None, 5 or 6), written out
HAND_ALL = {"src_pos": [0, 300], "src_var": [0, 1], "src_last": [2, 303], "sink_pos": [300, 600], "sink_var": [1, 0], "br_off": [0, 3, 5],
            "br_pos": [100, 200, NONE, 400, 500], "br_var": [1, 0, NONE, 0, 1], "br_nodes": [2, 5, 0, 1, 1], "br_cov": [11, 21, 0, 41, 51], "br_seq_off": [0, 2, 7, 7, 8, 9],
            "br_sup_in": [1000, 1001, 1002, 1005, 1006], "br_sup_out": [1003, 1004, 1002, 1007, 1008], "seq": b"CG" + b"GTACG" + b"A" + b"C"}
# at max_nodes 4 (one below the longest branch) only the second bubble is left
HAND_SHORT = {"src_pos": [300], "src_var": [1], "src_last": [303], "sink_pos": [600], "sink_var": [0], "br_off": [0, 2],
              "br_pos": [400, 500], "br_var": [0, 1], "br_nodes": [1, 1], "br_cov": [41, 51], "br_seq_off": [0, 1, 2], "br_sup_in": [1005, 1006], "br_sup_out": [1007, 1008], "seq": b"AC"}
HAND_TSV = (b"u7_0_0\tu7_300_1\t2\t300\t3\tu7_100_1,u7_200_0,*\t2,5,0\t11,21,0\t1000,1001,1002\t1003,1004,1002\tCG,GTACG,*\n"
            b"u7_300_1\tu7_600_0\t303\t600\t2\tu7_400_0,u7_500_1\t1,1\t41,51\t1005,1006\t1007,1008\tA,C\n")


# ---- the units -----------------------------------------------------------------------------------------------------------------------------

class BUnit:
    def __init__(self, name, unit, windows, want, coverage=1, iv=EU.LU.IV, support=False):
        """windows: [(lo, hi, threshold)]; want: [(description, window, fn(b, t) -> bool)] on the model's bubbles b of the window's table t; support: the GPU file also
        compares the rows' support on this unit"""
        self.name, self.unit, self.windows, self.want, self.coverage, self.iv, self.support = name, unit, list(windows), list(want), coverage, iv, support


C0, STEP, NB = 1000, 3, 300          # chain: bubble i forks at C0 + 3 i (a deletion of one base), its branch segment is C0 + 3 i + 1, its sink heads C0 + 3 i + 2


def unit_chain():
    """300 deletion bubbles in a row, each one's sink the next one's source (a sink runs on to the next fork, so a bubble adds two segments: 601 segments, 900 links,
    600 branch rows): over the edges of wavefronts and of 256-thread blocks in segments, bubbles and rows.  The windows cut the first bubbles at every border that matters."""
    end = C0 + STEP * NB
    ps = cover(C0 - 300, end + 300) + [dele(C0 + STEP * i, [1]) for i in range(NB)]
    whole = (0, 6 * 1024, 1)
    X = C0 + STEP * 5          # a bubble in the middle of the front: source's last position X, sink's head X + 2
    wins = [whole, (0, 6 * 1024, 0), (C0 - 200, X + 1, 1), (C0 - 200, X + 2, 1), (C0 - 200, X + 3, 1), (C0 - 200, X + 4, 1), (X, end + 200, 1), (X + 1, end + 200, 1), (X - 1, end + 200, 1),
            (X, X, 1), (C0 - 250, C0 - 50, 1), (C0 - 200, C0 + STEP * 70, 1), (C0 + 1, C0 + STEP * 129, 1)]

    def n_bub(k):
        return lambda b, t: b["n_bubbles_all"] == k and b["n_forks"] == k + b["n_tip"]
    want = [("300 bubbles of two rows, one direct and one of a single node, each sink the next source", whole,
             lambda b, t: b["n_bubbles_all"] == NB and b["n_forks"] == NB and len(b["br_pos"]) == 2 * NB and b["br_nodes"] == [1, 0] * NB and b["longest_branch"] == 1
             and b["src_pos"][1:] == b["sink_pos"][:-1] and b["n_segs"] == 2 * NB + 1),
            ("a window that ends on the sink's head position: the source keeps one link, no fork", (C0 - 200, X + 2, 1), lambda b, t: b["n_forks"] == 5 and b["n_bubbles_all"] == 5),
            ("a window that ends one before", (C0 - 200, X + 1, 1), lambda b, t: b["n_forks"] == 5 and b["n_bubbles_all"] == 5),
            ("a window that ends one behind: the sink is a segment of one node", (C0 - 200, X + 3, 1),
             lambda b, t: b["n_bubbles_all"] == 6 and b["n_forks"] == 6 and b["sink_pos"][-1] == X + 2 and t["n_nodes"][-1] == 1),
            ("a window that starts at a source's last position", (X, end + 200, 1), lambda b, t: b["n_bubbles_all"] == NB - 5 and b["src_pos"][0] == X and b["src_last"][0] == X),
            ("a window that starts one behind it", (X + 1, end + 200, 1), lambda b, t: b["n_bubbles_all"] == NB - 6 and b["src_pos"][0] == X + 1 and b["src_last"][0] == X + STEP),
            ("the empty window", (X, X, 1), lambda b, t: b["n_segs"] == 0 and b["n_forks"] == 0),
            ("a window without links", (C0 - 250, C0 - 50, 1), lambda b, t: b["n_segs"] == 1 and b["n_links"] == 0),
            ("70 bubbles: more than a wavefront of them", (C0 - 200, C0 + STEP * 70, 1), n_bub(70))]
    return BUnit("chain", Unit(6 * 1024, ps), wins, want, support=True)


XS, XD = 2048, 4096          # kinds: the substitution forks at XS, the two deletions at XD


def unit_kinds():
    """A bubble of two segment branches whose second branch has coverage 1 (three reads delete XS + 1, one deletes XS + 2 and nobody steps from XS + 1 to XS + 2): a
    bubble at threshold 1, no fork at 2.  Two deletions of different length at XD: XD -> XD + 1, XD + 2 and XD + 4, whose exits differ."""
    ps = [dele(XS, [1])] * 3 + [dele(XS + 1, [1])]
    ps += cover(XD - 200, XD + 200) + [dele(XD, [1]), dele(XD, [3])]
    ws1, ws2, wd = (XS - 100, XS + 100, 1), (XS - 100, XS + 100, 2), (XD - 100, XD + 100, 1)
    wins = [ws1, ws2, wd, (0, 6 * 1024, 1), (0, 6 * 1024, 0), (XS - 100, XS + 3, 1), (XS, XS + 4, 1)]
    want = [("a substitution: two segment branches of one node, coverage 3 and 1", ws1,
             lambda b, t: b["n_bubbles_all"] == 1 and b["n_forks"] == 1 and b["br_pos"] == [XS + 1, XS + 2] and b["br_nodes"] == [1, 1] and sorted(b["br_cov"]) == [1, 3]
             and b["src_last"] == [XS] and b["sink_pos"] == [XS + 3]),
            ("no fork at threshold 2", ws2, lambda b, t: b["n_forks"] == 0 and b["n_segs"] >= 1),
            ("two deletions of different length: SINKS_DIFFER", wd, lambda b, t: b["n_sinks_differ"] == 1 and b["n_forks"] == 1),
            ("the substitution cut in front of its sink: a TIP", (XS - 100, XS + 3, 1), lambda b, t: b["n_tip"] == 1 and b["n_forks"] == 1)]
    return BUnit("kinds", Unit(6 * 1024, ps), wins, want, support=True)


def unit_plain():
    """A unit without links: one strand."""
    w = (0, 4096, 1)
    return BUnit("plain", Unit(4096, cover(1000, 1500)), [w, (1100, 1200, 1), (0, 0, 1)], [("one segment, no link", w, lambda b, t: b["n_segs"] == 1 and b["n_links"] == 0 and b["n_forks"] == 0)])


def unit_pruned():
    """edge_units' overflow_pruned shape at its own coverage 4: of the source's nine successors only some survive the threshold, and a branch segment whose own
    successor is pruned is a TIP the threshold made."""
    c = EU.case_overflow_pruned()
    x = EU._at(0, 20)
    w4, w1 = (0, 6 * 1024, 4), (0, 6 * 1024, 1)
    return BUnit("edge_overflow_pruned", c.unit, [w4, w1, (x - 100, x + 200, 4)],
                 [("a TIP at threshold 4", w4, lambda b, t: b["n_tip"] >= 1), ("the threshold made it: fewer TIPs, or none, at 1", w1, lambda b, t: b["n_forks"] >= 1)], coverage=4)


def units():
    return [unit_chain(), unit_kinds(), unit_plain(), unit_pruned()]
