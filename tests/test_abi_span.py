"""The C layout of the pair-span structs (include/agx.h) against their ctypes mirrors, and agx_stats' two new fields at its end (CPU only): a small program compiled
against the header prints sizes and offsets."""
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
    printf("%zu %zu %zu\n", sizeof(agx_pair_span), sizeof(agx_walk_span), sizeof(agx_stats));
    printf("%zu %zu %zu %zu\n", offsetof(agx_stats, ms_edge_reads), offsetof(agx_stats, ms_pair_span), offsetof(agx_stats, ms_walk_span), offsetof(agx_pair_span, span));
    printf("%zu %zu %zu %zu\n", offsetof(agx_walk_span, n_steps_not_forward), offsetof(agx_walk_span, iv_rec), offsetof(agx_walk_span, track_off), offsetof(agx_walk_span, step));
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi_span")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    return [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]


def test_struct_sizes(c_layout):
    assert c_layout[0] == [ctypes.sizeof(A.PairSpan), ctypes.sizeof(A.WalkSpan), ctypes.sizeof(A.Stats)]
    assert ctypes.sizeof(A.PairSpan) == 2 * 4 + 3 * 8 + 2 * 8
    assert ctypes.sizeof(A.WalkSpan) == 2 * 4 + 4 * 8 + 12 * 8 + 2 * 4 + 8 + 8 + 3 * 8


def test_field_offsets(c_layout):
    assert c_layout[1] == [A.Stats.ms_edge_reads.offset, A.Stats.ms_pair_span.offset, A.Stats.ms_walk_span.offset, A.PairSpan.span.offset]
    assert c_layout[2] == [A.WalkSpan.n_steps_not_forward.offset, A.WalkSpan.iv_rec.offset, A.WalkSpan.track_off.offset, A.WalkSpan.step.offset]


def test_stats_grew_at_its_end_only():
    names = [n for n, _ in A.Stats._fields_]
    assert names[-3:] == ["ms_edge_reads", "ms_pair_span", "ms_walk_span"]
    assert A.Stats.ms_pair_span.offset == A.Stats.ms_edge_reads.offset + 8 and A.Stats.ms_walk_span.offset + 8 == ctypes.sizeof(A.Stats)


def test_exports_and_methods():
    for name in ("agx_unit_pair_span", "agx_pair_span_free", "agx_unit_walk_span", "agx_walk_span_free", "agx_walk_span_bed"):
        assert name in A.EXPORTS
    assert callable(A.Unit.pair_span) and callable(A.Unit.walk_span) and callable(A.span_bed)
