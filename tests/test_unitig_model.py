"""The unitig model (tests/unitig_model.py) on hand-made graphs, each against its exact GFA text (CPU only)."""
from unitig_model import graph_from_lists, unit_gfa

C = 5
V = (0, 0, 0, 0, 0)
REF = b"ACGTACGTACGT"


def node(cov=10, votes=(9, 0, 0, 0, 0), cid=None):
    return (cid, cov, votes)


def test_chain():
    g = graph_from_lists([1, 1, 1], [node(10, (9, 0, 0, 0, 0)), node(11, (0, 8, 0, 0, 0)), node(12, (0, 0, 7, 0, 0))], [(0, 1), (1, 2)])
    assert unit_gfa(g, C, REF, 0) == b"S\tu0_0_0\tACG\tLN:i:3\tKC:i:33\tpe:i:2\n"


def test_fork():
    g = graph_from_lists([1, 1, 2, 1], [node(), node(), node(votes=(0, 5, 0, 0, 0)), node(votes=(0, 0, 0, 5, 0)), node()], [(0, 1), (1, 2), (1, 3), (3, 4)])
    assert unit_gfa(g, C, REF, 3) == (b"S\tu3_0_0\tAA\tLN:i:2\tKC:i:20\tpe:i:1\n"
                                      b"S\tu3_2_0\tC\tLN:i:1\tKC:i:10\tpe:i:2\n"
                                      b"S\tu3_2_1\tTA\tLN:i:2\tKC:i:20\tpe:i:3\n"
                                      b"L\tu3_0_0\t+\tu3_2_0\t+\t0M\n"
                                      b"L\tu3_0_0\t+\tu3_2_1\t+\t0M\n")


def test_bubble():
    g = graph_from_lists([1, 2, 1], [node(), node(votes=(0, 1, 0, 0, 0)), node(votes=(0, 0, 1, 0, 0)), node(votes=(0, 0, 0, 1, 0))], [(0, 1), (0, 2), (1, 3), (2, 3)])
    assert unit_gfa(g, C, REF, 0) == (b"S\tu0_0_0\tA\tLN:i:1\tKC:i:10\tpe:i:0\n"
                                      b"S\tu0_1_0\tC\tLN:i:1\tKC:i:10\tpe:i:1\n"
                                      b"S\tu0_1_1\tG\tLN:i:1\tKC:i:10\tpe:i:1\n"
                                      b"S\tu0_2_0\tT\tLN:i:1\tKC:i:10\tpe:i:2\n"
                                      b"L\tu0_0_0\t+\tu0_1_0\t+\t0M\n"
                                      b"L\tu0_0_0\t+\tu0_1_1\t+\t0M\n"
                                      b"L\tu0_1_0\t+\tu0_2_0\t+\t0M\n"
                                      b"L\tu0_1_1\t+\tu0_2_0\t+\t0M\n")


def test_pruned_middle_node_splits_a_chain():
    g = graph_from_lists([1, 1, 1, 1], [node(), node(), node(cov=4), node()], [(0, 1), (1, 2), (2, 3)])
    assert unit_gfa(g, C, REF, 0) == (b"S\tu0_0_0\tAA\tLN:i:2\tKC:i:20\tpe:i:1\n"
                                      b"S\tu0_3_0\tA\tLN:i:1\tKC:i:10\tpe:i:3\n")


def test_node_with_six_out_edges():
    # (one edge listed twice, as the overflow list can; it counts once)
    g = graph_from_lists([1, 6], [node()] + [node(votes=(0, 0, 0, 0, 3))] * 6, [(0, j) for j in range(1, 7)] + [(0, 4)])
    want = b"S\tu1_0_0\tA\tLN:i:1\tKC:i:10\tpe:i:0\n" + b"".join(b"S\tu1_1_%d\tN\tLN:i:1\tKC:i:10\tpe:i:1\n" % v for v in range(6)) + \
        b"".join(b"L\tu1_0_0\t+\tu1_1_%d\t+\t0M\n" % v for v in range(6))
    assert unit_gfa(g, C, REF, 1) == want


def test_zero_vote_contig_node_takes_the_reference_base():
    g = graph_from_lists([1, 1, 1], [node(), node(cov=0, votes=V, cid=7), node(votes=(0, 0, 0, 4, 0))], [(0, 1), (1, 2)])
    assert unit_gfa(g, C, REF, 0) == b"S\tu0_0_0\tACT\tLN:i:3\tKC:i:20\tpe:i:2\n"


def test_vote_tie():
    g = graph_from_lists([1, 1, 1, 1], [node(votes=(0, 3, 3, 0, 0)), node(votes=(0, 0, 2, 2, 2)), node(votes=(1, 1, 1, 1, 1)), node(votes=(0, 0, 0, 4, 4))],
                         [(0, 1), (1, 2), (2, 3)])
    assert unit_gfa(g, C, REF, 0) == b"S\tu0_0_0\tCGAT\tLN:i:4\tKC:i:40\tpe:i:3\n"


def test_empty_unit():
    assert unit_gfa(graph_from_lists([0, 0], [], []), C, REF, 0) == b""
    assert unit_gfa(graph_from_lists([1, 1], [node(cov=1), node(cov=2)], [(0, 1)]), C, REF, 0) == b""
