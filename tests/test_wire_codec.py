"""The compact wire forms of the hit and side records (csrc/agx_core.h "compact wire forms") on the CPU: every record comes back exactly.

tests/wire_shim.cpp packs arrays handed in from numpy the way the staging does (blocks of 64 hits with an escape list and a list of extra words; a side's two counts as
bytes with a list of the sides that need more) and unpacks them the way the device's lanes do.  What must come out is the input, byte for byte; the counts of escapes
say that a case took the path it is here for.  The widths asserted here are the format's: 12 bits of left-mate offset above the block's base, 12 bits of signed distance
to the other mate, 24 bits of offset for the one position of a hit with a side record.  (The run records cross as they are: no case for them here.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import forms_shim
from forms_shim import BLOCK, DUP, L, LEFT2, LISTED, REV1, REV2, RUNS1, RUNS2, WHIT, WSIDE, plain_hits  # noqa: F401  (the record types and hits shared with tests/test_stage_forms.py)

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "wire_shim.cpp")


@pytest.fixture(scope="module")
def shim():
    return forms_shim.lib()      # (compiled alone with -Wall -Wextra -Werror; as a program of its own under the sanitizers: the last test)



def hit(a, b, row=0, length=L, flags=0, back=0):
    return (a, b, row, length, flags, back)


def hits_of(records):
    return np.array(records, WHIT) if len(records) else np.zeros(0, WHIT)


def round_trip(shim, hits, maxlen=L):
    """(escapes, extra words, blocks) of the packing; asserts that both ways back give the input."""
    n = len(hits)
    hits = np.ascontiguousarray(hits)
    blocks, esc, ext, counts = np.zeros(n // 64 + 1, BLOCK), np.zeros(n + 1, WHIT), np.zeros(n + 1, np.uint32), np.zeros(2, np.uint32)
    shim.agx_wire_pack_hits(hits.ctypes.data, n, maxlen, 3, blocks.ctypes.data, esc.ctypes.data, ext.ctypes.data, counts.ctypes.data)      # (the product's packer, on three threads)
    for back in (shim.agx_wire_unpack_hits, shim.agx_wire_unpack_hits_serial):
        out = np.zeros(n + 1, WHIT)
        out[n] = (7, 7, 7, 7, 7, 7)
        back(blocks.ctypes.data, n, maxlen, esc.ctypes.data, ext.ctypes.data, out.ctypes.data)
        assert out[:n].tobytes() == hits.tobytes()
        assert tuple(out[n]) == (7, 7, 7, 7, 7, 7), "a write behind the last record"
    return int(counts[0]), int(counts[1]), blocks


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129])
def test_block_edges(shim, n):
    h = plain_hits(n, seed=n)
    n_esc, n_ext, blocks = round_trip(shim, h)
    assert n_esc == 0 and n_ext == int(np.count_nonzero(h["flags"] & (RUNS1 | RUNS2)))
    if n > 64:
        assert blocks["esc"][1] == 0 and blocks["ext"][1] == int(np.count_nonzero(h["flags"][:64] & (RUNS1 | RUNS2))), "the second block's header names its first extra word"


def test_all_escaped_and_none_and_the_outer_lanes(shim):
    h = plain_hits(192)
    h["back"][:64] = 1                       # block 0: every hit escapes
    h["back"][128], h["len"][191] = 255, L - 1      # block 2: lane 0 and lane 63
    n_esc, _, blocks = round_trip(shim, h)
    assert n_esc == 66 and list(blocks["esc"][:3]) == [0, 64, 64]
    assert not blocks["word"][0].any() and (blocks["word"][1] & 0xC0 == 0xC0).all(), "an escaped slot is zero, a compact one carries both marks"
    assert blocks["word"][2][0] == 0 and blocks["word"][2][63] == 0 and blocks["word"][2][1:63].all()


@pytest.mark.parametrize("left2", [False, True])
def test_offsets_at_the_last_value_that_fits(shim, left2):
    """The left mate 4095 above the base fits, 4096 does not; the other mate 2047 above and 2048 below the left one fits, 2048 above and 2049 below do not."""
    base = 100000

    def one(left, other):
        return hit(other, left, flags=LEFT2) if left2 else hit(left, other)

    cases = [(one(base + 4095, base + 4095 + 300), 0), (one(base + 4096, base + 4096 + 300), 1), (one(base + 10, base + 10 + 2047), 0), (one(base + 10, base + 10 + 2048), 1),
             (one(base + 3000, base + 3000 - 2048), 0), (one(base + 3000, base + 3000 - 2049), 1)]
    for record, want in cases:
        n_esc, n_ext, blocks = round_trip(shim, hits_of([one(base, base + 300), record]))
        assert (n_esc, n_ext) == (want, 0) and blocks["base"][0] == base, record
    # the one position of a hit with a side record: 24 bits above the base
    for off, want in ((0xFFFFFF, 0), (0x1000000, 1)):
        n_esc, n_ext, _ = round_trip(shim, hits_of([hit(base, base + 300), hit(5, base + off, flags=RUNS1), hit(base + off, 5, flags=RUNS2)]))
        assert (n_esc, n_ext) == (2 * want, 2 - 2 * want)


def test_every_flag_combination(shim):
    records = []
    for f in range(64):
        a = 77 if f & RUNS1 else 9000 + f
        b = (0 if f & RUNS1 else 78) if f & RUNS2 else 9300 + f
        records.append(hit(a, b, row=f * 1000003, flags=f))
    n_esc, n_ext, _ = round_trip(shim, hits_of(records))
    assert n_esc == 0 and n_ext == 48
    # a flag bit beyond the six, and a second side field that is not the loaders' zero but small: the first escapes, the second travels in the 24 bits
    n_esc, n_ext, _ = round_trip(shim, hits_of([hit(9000, 9300, flags=64), hit(9000, 9300, flags=128), hit(3, 12345, flags=RUNS1 | RUNS2), hit(3, 1 << 24, flags=RUNS1 | RUNS2)]))
    assert (n_esc, n_ext) == (3, 1)


def test_len_back_and_side_index(shim):
    rows = [hit(9000, 9300), hit(9001, 9301, length=L - 1), hit(9002, 9302, length=L + 1), hit(9003, 9303, back=1), hit(9004, 9304, back=255),
            hit(0, 9305, flags=RUNS1), hit(0xFFFFFFFE, 9306, flags=RUNS1), hit(9007, 0, flags=RUNS2), hit(9008, 0xFFFFFFFE, flags=RUNS2 | LEFT2)]
    n_esc, n_ext, _ = round_trip(shim, hits_of(rows))
    assert (n_esc, n_ext) == (4, 4)
    for maxlen in (255, 256):      # (the hit records hold len whole: nothing changes at a byte's edge)
        n_esc, _, _ = round_trip(shim, hits_of([hit(9000, 9300, length=maxlen), hit(9001, 9301, length=maxlen - 1)]), maxlen=maxlen)
        assert n_esc == 1


def test_hits_the_block_base_cannot_reach(shim):
    h = plain_hits(128)
    simple = (h["flags"] & (RUNS1 | RUNS2)) == 0
    far = np.arange(128) % 2 == 1
    h["a"] = np.where(simple & far, h["a"] + 70000, h["a"])      # every other hit 70 000 positions on (its mate with it)
    h["b"] = np.where(simple & far, h["b"] + 70000, h["b"])
    n_esc, _, _ = round_trip(shim, h)
    assert n_esc == int(np.count_nonzero(simple & far))


def test_any_record_comes_back(shim):
    rnd = np.random.RandomState(5)
    raw = rnd.randint(0, 256, 100000 * WHIT.itemsize, dtype=np.uint8)
    h = raw.view(WHIT).copy()
    n_esc, _, _ = round_trip(shim, h)
    assert n_esc > 90000      # (random records all but never fit)
    h["len"], h["back"] = L, 0
    h["flags"] &= 63
    h["b"] = np.where((h["flags"] & (RUNS1 | RUNS2)) == 0, h["a"] + rnd.randint(-3000, 3000, len(h)).astype(np.uint32), h["b"])      # all 32 bits of a, b and row in play, some mates in reach
    n_esc, n_ext, _ = round_trip(shim, h)
    assert 0 < n_esc < len(h) and n_ext > 0


def sides_round_trip(shim, sides):
    n = len(sides)
    sides = np.ascontiguousarray(sides)
    counts, listed, nl, first = np.zeros(n + 1, np.uint16), np.zeros(n + 1, LISTED), ctypes.c_uint32(0), ctypes.c_uint32(0)
    ok = shim.agx_wire_pack_sides(sides.ctypes.data, n, counts.ctypes.data, listed.ctypes.data, ctypes.byref(nl), ctypes.byref(first))
    if not ok:
        return None
    out = np.zeros(n, WSIDE)
    shim.agx_wire_unpack_sides(counts.ctypes.data, n, listed.ctypes.data, nl.value, first.value, out.ctypes.data)
    assert out.tobytes() == sides.tobytes()
    return nl.value


def sides_of(counts, first=0):
    s, at = np.zeros(len(counts), WSIDE), first
    for i, (n1, n2) in enumerate(counts):
        s[i] = (at if n1 else 0, at + n1 if n2 else 0, n1 | n2 << 16)      # (a mate without runs names no place in the pool: the loaders' zero)
        at += n1 + n2
    return s


def test_sides(shim):
    assert sides_round_trip(shim, sides_of([])) == 0
    assert sides_round_trip(shim, sides_of([(1, 1), (255, 0), (0, 255), (2, 3)], first=11)) == 0
    assert sides_round_trip(shim, sides_of([(1, 1), (256, 1), (1, 256), (255, 255), (65535, 0), (0, 65535), (65535, 65535), (3, 0)])) == 6
    rnd = np.random.RandomState(2)
    many = [(int(a), int(b)) for a, b in zip(rnd.randint(0, 300, 5000), rnd.randint(1, 6, 5000))]
    assert sides_round_trip(shim, sides_of(many)) == sum(1 for a, _ in many if a > 255)


def test_a_run_pool_out_of_side_order_sends_the_records(shim):
    s = sides_of([(2, 1), (1, 3), (2, 2)])
    assert sides_round_trip(shim, s) == 0
    assert sides_round_trip(shim, sides_of([(2, 0), (0, 3), (1, 1)], first=5)) == 0
    z = sides_of([(2, 0), (0, 3), (1, 1)])
    z["runs2"][0] = 2                                   # the field of a mate without runs is not the zero: nothing the device would rebuild
    assert sides_round_trip(shim, z) is None
    for field, i in (("runs1", 1), ("runs2", 1), ("runs1", 2)):
        t = s.copy()
        t[field][i] += 1
        assert sides_round_trip(shim, t) is None
    assert sides_round_trip(shim, s[::-1].copy()) is None
    big = sides_of([(65535, 65535)] * 3, first=0xFFFFFFFF - 5 * 65535)      # a pool that would end beyond 2^32 runs
    assert sides_round_trip(shim, big) is None


def test_the_shim_as_a_program_of_its_own_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wire_shim_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DAGX_WIRE_SHIM_MAIN", "-o", exe, SHIM])
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip() == "wire shim: ok"
