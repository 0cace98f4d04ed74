"""The look-back of the one-launch scan on the CPU, and the arithmetic of the sizes tests/test_gpu_primitives.py runs.

agx_scan_window_take (csrc/agx_core.h) is what a lane of agx_k_scan_lookback takes from a window of 64 predecessors; tests/scan_shim.cpp runs it over descriptor arrays
this file sets to any state and replays a block's whole look-back serially.  tests/scan_model.py says what must come out: "walk back from b - 1, add what you meet,
stop behind the first prefix".  The window counts are asserted from that model, so a case that is here for the second window says so itself.
The last tests hold the table of scan sizes against the arm each size is named for: nb, nb2, launches, and the iterations of a workgroup at a capped grid."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import scan_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "scan_shim.cpp")
U32, U64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
AGG, PFX = M.AGG, M.PFX
BLOCKS = (0, 1, 63, 64, 65, 127, 128, 129, 200)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scan_shim") / "libscan_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so, SHIM])
    L = ctypes.CDLL(so)
    L.agx_scan_window_shim.argtypes = [U64, ctypes.c_longlong, U32, ctypes.POINTER(ctypes.c_int)]
    L.agx_scan_lookback_shim.argtypes = [U64, ctypes.c_uint32, U32, U32]
    return L


def pack(flags, values):
    return np.array([f | (int(v) & 0xFFFFFFFF) for f, v in zip(flags, values)], np.uint64)


def run_window(shim, flags, values, hi):
    """The window hi, hi - 1, .., hi - 63 of the descriptors: (parts, last) from the shim and from the model."""
    desc = pack(flags, values)
    parts, last = np.zeros(64, np.uint32), ctypes.c_int(-1)
    assert shim.agx_scan_window_shim(desc.ctypes.data_as(U64), hi, parts.ctypes.data_as(U32), ctypes.byref(last)) == 0
    lanes = [(flags[hi - l], values[hi - l]) if hi - l >= 0 else (PFX, 0) for l in range(64)]      # in front of block 0: a prefix of 0
    want, want_last = M.window([f for f, _ in lanes], [v for _, v in lanes])
    return [int(p) for p in parts], bool(last.value), want, want_last


def run_lookback(shim, flags, values, b):
    desc = pack(flags, values) if len(flags) else np.zeros(1, np.uint64)
    excl, windows = ctypes.c_uint32(0xDEAD), ctypes.c_uint32(0xDEAD)
    assert shim.agx_scan_lookback_shim(desc.ctypes.data_as(U64), b, ctypes.byref(excl), ctypes.byref(windows)) == 0
    return excl.value, windows.value


@pytest.mark.parametrize("at", [0, 1, 31, 32, 62, 63, None])
def test_window_stops_behind_the_nearest_prefix(shim, at):
    """hi = 200: all 64 lanes are real blocks.  Behind the nearest prefix lie junk values under both flags, a second prefix among them: none of it may count."""
    rnd = np.random.RandomState(3)
    n, hi = 201, 200
    values = rnd.randint(1, 1 << 32, n, dtype=np.uint64)
    flags = [AGG] * n
    if at is not None:
        flags[hi - at] = PFX
        for lane in range(at + 1, 64):
            flags[hi - lane] = PFX if lane % 3 == 0 else AGG
    got, last, want, want_last = run_window(shim, flags, values, hi)
    assert want_last == (at is not None) and sum(1 for p in want if p) == (64 if at is None else at + 1), "the model itself: %d lanes count" % (64 if at is None else at + 1)
    assert got == want and last == want_last


@pytest.mark.parametrize("hi", [0, 1, 62, 63, 64])
def test_lanes_in_front_of_block_0_are_a_prefix_of_zero(shim, hi):
    rnd = np.random.RandomState(hi)
    values = rnd.randint(1, 1 << 32, hi + 1, dtype=np.uint64)
    flags = [AGG] * (hi + 1)                                        # block 0 an aggregate too: only the lanes in front of it can end the walk
    got, last, want, want_last = run_window(shim, flags, values, hi)
    assert want_last == (hi < 63) and sum(1 for p in want if p) == min(hi + 1, 64)
    assert got == want and last == want_last
    flags[0] = PFX                                                   # block 0 as it is in a run
    got, last, want, want_last = run_window(shim, flags, values, hi)
    assert want_last == (hi < 64)
    assert got == want and last == want_last


def test_a_window_of_all_ones_wraps(shim):
    flags, values = [AGG] * 64, [0xFFFFFFFF] * 64
    got, last, want, want_last = run_window(shim, flags, values, 63)
    assert got == want == [0xFFFFFFFF] * 64 and not last and not want_last
    assert sum(got) & 0xFFFFFFFF == (-64) & 0xFFFFFFFF
    excl, windows = run_lookback(shim, flags + [AGG], values + [0], 64)
    assert (excl, windows) == ((-64) & 0xFFFFFFFF, 1)


def test_a_prefix_on_lane_0_hides_everything_behind_it(shim):
    rnd = np.random.RandomState(11)
    values = rnd.randint(1, 1 << 32, 100, dtype=np.uint64)
    flags = [PFX if rnd.randint(0, 2) else AGG for _ in range(100)]
    flags[99] = PFX
    got, last, want, want_last = run_window(shim, flags, values, 99)
    assert want == [int(values[99])] + [0] * 63 and want_last
    assert got == want and last


def arrangement(name, b, rnd):
    """Descriptors 0 .. b - 1 in front of block b: flags by the arrangement, values random (a prefix's value need not be the sum of what lies behind it: the walk
    must not look there)."""
    flags = [AGG] * b
    if name == "only_block_0":
        pass
    elif name == "prefix_64_behind":
        if b >= 64:
            flags[b - 64] = PFX
    elif name == "prefix_65_behind":
        if b >= 65:
            flags[b - 65] = PFX
    elif name == "every_predecessor":
        flags = [PFX] * b
    elif name == "none_at_all":                                      # not a state of a run (block 0 always publishes a prefix): the walk leaves the array at its front
        return flags, rnd.randint(0, 1 << 32, b, dtype=np.uint64)
    if b:
        flags[0] = PFX
    return flags, rnd.randint(0, 1 << 32, b, dtype=np.uint64)


@pytest.mark.parametrize("b", BLOCKS)
@pytest.mark.parametrize("name", ["only_block_0", "prefix_64_behind", "prefix_65_behind", "every_predecessor", "none_at_all"])
def test_replayed_lookback_matches_the_model(shim, name, b):
    flags, values = arrangement(name, b, np.random.RandomState(b))
    want, read = M.lookback(flags, values, b)
    windows = M.windows_read(read)
    if name in ("only_block_0", "none_at_all"):
        assert read == b and windows == (b + 63) // 64, "the model itself: only block 0 a prefix takes ceil(b / 64) windows"
    elif name == "prefix_64_behind" and b >= 64:
        assert read == 64 and windows == 1, "the model itself: a prefix on the window's last lane ends the walk there"
    elif name == "prefix_65_behind" and b >= 65:
        assert read == 65 and windows == 2, "the model itself: a prefix one behind the window takes a second window"
    elif name == "every_predecessor":
        assert read == min(b, 1) and windows == min(b, 1)
    assert run_lookback(shim, flags, values, b) == (want, windows)


def test_unpublished_descriptor_is_reported_not_summed(shim):
    """The kernel waits for a descriptor of 0; the replay says so instead of taking its value."""
    flags, values = [PFX, AGG, 0, AGG], [5, 6, 7, 8]
    desc = pack(flags, values)
    excl, windows = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert shim.agx_scan_lookback_shim(desc.ctypes.data_as(U64), 4, ctypes.byref(excl), ctypes.byref(windows)) == -1
    assert run_lookback(shim, flags[:2], values[:2], 2) == (11, 1)


def test_replay_agrees_with_a_scan_of_the_block_totals(shim):
    """Descriptors as a finished run leaves them, and as a seeded run starts: every look-back gives the exclusive prefix of the totals."""
    rnd = np.random.RandomState(5)
    nb = 301
    totals = np.where(rnd.randint(0, 2, nb) == 0, 0xFFFFFFFF, rnd.randint(0, 1 << 32, nb, dtype=np.uint64)).astype(np.uint64)
    incl = np.cumsum(totals, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    for state in ("finished", "seeded", "mixed"):
        flags = [PFX if state == "finished" or b == 0 or (state == "mixed" and rnd.randint(0, 70) == 0) else AGG for b in range(nb)]
        values = [incl[b] if flags[b] == PFX else totals[b] for b in range(nb)]
        for b in range(nb + 1):
            excl, windows = run_lookback(shim, flags, values, b)
            assert excl == (int(incl[b - 1]) if b else 0), (state, b)
            assert windows == M.windows_read(M.lookback(flags, values, b)[1]), (state, b)
        if state == "seeded":
            assert run_lookback(shim, flags, values, 300)[1] == 5, "a seeded run walks over several windows"


# ---- the case table of tests/test_gpu_primitives.py ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(M.SCAN_SIZES))
def test_every_scan_size_reaches_the_arm_it_is_named_for(n):
    nb, nb2, launches = M.SCAN_SIZES[n]
    assert M.levels(n) == (nb, nb2, launches)
    assert (nb - 1) * 4096 < n + 1 <= nb * 4096 and (nb2 - 1) * 4096 < nb <= nb2 * 4096
    assert launches == (1 if n + 1 <= 4096 else 3 if n + 1 <= 4096 * 4096 else 5)
    assert M.tmp_words(n) == 2 * (nb + 1) + 2 * (nb2 + 1)


def test_the_sizes_sit_on_both_sides_of_every_level():
    s = M.SCAN_SIZES
    assert s[4095][2] == 1 and s[4096][2] == 3, "n + 1 = 4096 is the last one-block scan"
    assert s[16777215][2] == 3 and s[16777216][2] == 5, "n + 1 = 4096^2 is the last two-level scan"
    assert s[16777216][:2] == (4097, 2) and 4097 - 4096 == 1, "the second block of level two holds one sum"
    assert [p < 16777216 for p in M.STEP_AT] == [True, True, True, False], "the last step lies in block 4096: only the three-level sizes hold it"
    assert [n for n in s if n > M.ALL_PATTERNS_UP_TO] == [16777214, 16777215, 16777216, 16781312, 20000001]


@pytest.mark.parametrize("grid", [c for c in M.GRID_CAPS if c] + [1024])
def test_capped_block_counts_give_one_two_and_three_iterations(grid):
    blocks = M.capped_blocks(grid)
    assert blocks == ([grid - 1] if grid > 1 else []) + [grid, grid + 1, 2 * grid + 1]
    for nb in blocks:
        its = M.iterations(nb, grid)
        assert sum(its) == nb
        if nb == grid - 1:
            assert its == [1] * (grid - 1), "the last workgroup is not launched"
        elif nb == grid:
            assert its == [1] * grid
        elif nb == grid + 1:
            assert its == [2] + [1] * (grid - 1), "workgroup 0 takes a second block"
        else:
            assert its == [3] + [2] * (grid - 1), "workgroup 0 takes a third block, every other a second"
        n = M.n_for_blocks(nb)
        assert M.levels(n)[0] == nb and (n + 1) % 4096 == 1234, "the last block is partial"


@pytest.mark.parametrize("nb,windows", [(65, 1), (66, 2), (129, 2), (300, 5)])
def test_own_grid_block_counts_and_the_windows_of_their_last_block(nb, windows):
    """65 blocks: the last one's 64 predecessors fill one window exactly; 66 is the first count with a second window."""
    assert nb in M.OWN_GRID_BLOCKS
    n = M.n_for_blocks(nb)
    assert M.levels(n)[0] == nb
    flags = [PFX] + [AGG] * (nb - 2)                                 # the last block's predecessors as a seeded run starts
    assert M.windows_read(M.lookback(flags, [1] * (nb - 1), nb - 1)[1]) == windows
