"""The C layout of agx_bubbles (include/agx.h) against its ctypes mirror, the exports, and agx_stats, which the feature leaves as it was (CPU only): a small program
compiled against the header prints sizes and offsets."""
import ctypes
import os
import subprocess

import pytest

import aligngraph_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [n for n, _ in A.Bubbles._fields_] if hasattr(A, "Bubbles") else []
PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "agx.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(agx_bubbles), sizeof(agx_stats), offsetof(agx_stats, ms_walk_span));
    printf("%s\n", "FIELDS");
    return 0;
}
"""


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("abi_bubbles")
    src, exe = str(d / "layout.c"), str(d / "layout")
    with open(src, "w") as f:
        f.write(PROGRAM.replace('printf("%s\\n", "FIELDS");', "".join('printf("%%zu ", offsetof(agx_bubbles, %s));' % n for n in FIELDS) + 'printf("\\n");'))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    return [[int(v) for v in line.split()] for line in subprocess.check_output([exe]).decode().splitlines()]


def test_struct_sizes(c_layout):
    assert c_layout[0] == [ctypes.sizeof(A.Bubbles), ctypes.sizeof(A.Stats), A.Stats.ms_walk_span.offset]
    assert ctypes.sizeof(A.Bubbles) == 2 * 4 + 6 * 8 + 5 * 4 + 4 + 3 * 8 + 14 * 8      # (four bytes of padding in front of n_bases)


def test_every_field_offset(c_layout):
    assert len(FIELDS) == 30 and c_layout[1] == [getattr(A.Bubbles, n).offset for n in FIELDS]
    assert FIELDS[:8] == ["n_segs", "n_links", "n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared"] and FIELDS[-1] == "seq"


def test_the_time_is_the_calls_own_and_stats_stay():
    """The call's wall time is a field of agx_bubbles; agx_stats did not grow."""
    assert "ms" in FIELDS and "bytes_down" in FIELDS
    assert [n for n, _ in A.Stats._fields_][-1] == "ms_walk_span" and A.Stats.ms_walk_span.offset + 8 == ctypes.sizeof(A.Stats)


def test_exports_and_methods():
    for name in ("agx_unit_bubbles", "agx_unitigs_bubbles", "agx_bubbles_free", "agx_bubbles_tsv"):
        assert name in A.EXPORTS and hasattr(A.lib(), name)
    assert callable(A.Unit.bubbles) and callable(A.unitigs_bubbles) and callable(A.bubbles_tsv)
