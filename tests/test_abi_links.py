"""The C layout of agx_mate_links (include/agx.h) against its ctypes mirror, and agx_stats, which the feature leaves as it was (CPU only): a small program compiled against the
header prints sizes and offsets."""
import ctypes
import os
import subprocess

import pytest

import aligngraph_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "agx.h"
int main(void) {
    printf("%zu %zu\n", sizeof(agx_mate_links), sizeof(agx_stats));
    printf("%zu %zu\n", offsetof(agx_stats, ms_walk_span), offsetof(agx_mate_links, ms));
    printf("%zu %zu %zu %zu %zu %zu\n", offsetof(agx_mate_links, n_kept), offsetof(agx_mate_links, n_fragments), offsetof(agx_mate_links, n_links_all),
           offsetof(agx_mate_links, n_shadowed), offsetof(agx_mate_links, n_recs), offsetof(agx_mate_links, n_slots));
    printf("%zu %zu %zu %zu %zu %zu\n", offsetof(agx_mate_links, rec_inside), offsetof(agx_mate_links, rec_links_in), offsetof(agx_mate_links, a),
           offsetof(agx_mate_links, n_pairs), offsetof(agx_mate_links, len_sum), offsetof(agx_mate_links, hi_max));
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi_links")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    return [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]


def test_struct_sizes(c_layout):
    assert c_layout[0] == [ctypes.sizeof(A.MateLinks), ctypes.sizeof(A.Stats)]
    assert ctypes.sizeof(A.MateLinks) == 10 * 8 + 4 * 4 + 8 + 13 * 8


def test_field_offsets(c_layout):
    M = A.MateLinks
    assert c_layout[1] == [A.Stats.ms_walk_span.offset, M.ms.offset]
    assert c_layout[2] == [M.n_kept.offset, M.n_fragments.offset, M.n_links_all.offset, M.n_shadowed.offset, M.n_recs.offset, M.n_slots.offset]
    assert c_layout[3] == [M.rec_inside.offset, M.rec_links_in.offset, M.a.offset, M.n_pairs.offset, M.len_sum.offset, M.hi_max.offset]


def test_the_time_is_the_calls_own_and_stats_stay():
    """The call's wall time is a field of agx_mate_links, behind n_slots; agx_stats did not grow."""
    assert A.MateLinks.ms.offset == A.MateLinks.n_slots.offset + 4 and A.MateLinks.rec_inside.offset == A.MateLinks.ms.offset + 8
    assert [n for n, _ in A.Stats._fields_][-1] == "ms_walk_span" and A.Stats.ms_walk_span.offset + 8 == ctypes.sizeof(A.Stats)


def test_exports_and_methods():
    for name in ("agx_unit_mate_links", "agx_mate_links_free", "agx_mate_links_tsv"):
        assert name in A.EXPORTS
    assert callable(A.Unit.mate_links) and callable(A.links_tsv)
