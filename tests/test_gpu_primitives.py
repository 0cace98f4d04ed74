"""The primitives under every build and export, each against a plain reference: the exclusive scan in its two forms (numpy.cumsum, tests/scan_model.py), agx_k_zero
(zeros) and agx_k_copy_out (a byte copy), through the library's test hooks agx_test_scan, agx_test_zero and agx_test_copy_out.  The hooks run the product's own
launchers on the arrays given here and follow every device array with guard words that come back with it.

What every scan case asserts (check_scan): out[0 .. n] equals the model at every index; every guard word behind out, tmp and desc holds its pattern; for the one-launch
form every desc[b] is the prefix flag over the inclusive prefix of block b, the value the next block trusts; the answer is the same for two values of in[n]; and the
two forms agree.  The sizes and what each is there for: tests/scan_model.py, held by arithmetic in tests/test_scan_cases.py.

With seeded = 0 the number of windows a block's look-back walks over depends on how far its predecessors have come, which nothing outside the kernel can see: the
seeded cases (every descriptor an aggregate when the launch starts, so that a late block walks over all of them) and the CPU replay of tests/test_scan_cases.py are
what hold the walk over more than one window."""
import ctypes

import numpy as np
import pytest

import scan_model as M

pytestmark = pytest.mark.gpu

G = M.GUARD
U8, U32, U64 = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
TAILS = (0xDEADBEEF, 0)             # in[n]: junk, and the product's zero
GUARD64 = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def L():
    import aligngraph_amd as A
    assert A.device_count() > 0
    return A.lib()


def run_scan(L, form, a, grid_cap=0, seeded=0, streams=1):
    """One call of the hook: (out[streams][n + 1 + G], desc[streams][nb + G] or tmp[streams][words + G], the grid limit that held)."""
    n = len(a) - 1
    nb = M.levels(n)[0]
    out = np.zeros(streams * (n + 1 + G), np.uint32)
    desc = np.zeros(streams * (nb + G), np.uint64) if form == 1 else None
    tmp = np.zeros(streams * (M.tmp_words(n) + G), np.uint32) if form == 0 else None
    limit = ctypes.c_uint32(0)
    rc = L.agx_test_scan(0, form, a.ctypes.data_as(U32), n, out.ctypes.data_as(U32), grid_cap, seeded, streams,
                         desc.ctypes.data_as(U64) if form == 1 else None, tmp.ctypes.data_as(U32) if form == 0 else None, ctypes.byref(limit))
    assert rc == 0, "agx_test_scan: %d" % rc
    return out.reshape(streams, -1), (desc if form == 1 else tmp).reshape(streams, -1), limit.value


def first_difference(got, want, blocks=True):
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return None
    i = int(bad[0])
    if not blocks:
        return "%d of %d descriptors differ, the first that of block %d: %#x, the model has %#x" % (len(bad), len(want), i, got[i], want[i])
    return "%d of %d words differ, the first at index %d (block %d, word %d of it): %d, the model has %d" % (len(bad), len(want), i, i // M.BLOCK, i % M.BLOCK, got[i], want[i])


def check_scan(L, a, forms=(0, 1), grid_cap=0, seeded=0, streams=1, what=""):
    """a: the n + 1 input words (a[n] is overwritten with each tail in turn)."""
    n = len(a) - 1
    nb = M.levels(n)[0]
    a[n] = 0
    want = M.exclusive_scan(a)
    prefixes = M.block_prefixes(a)
    answers = []
    for tail in TAILS:
        a[n] = tail
        with_tail = prefixes.copy()
        with_tail[nb - 1] = (int(with_tail[nb - 1]) + tail) & 0xFFFFFFFF
        for form in forms:
            out, aux, _ = run_scan(L, form, a, grid_cap if form == 1 else 0, seeded if form == 1 else 0, streams)
            for s in range(streams):
                tag = "%s form %d, in[n] = %#x, stream %d" % (what, form, tail, s)
                assert first_difference(out[s, :n + 1], want) is None, tag + ": " + first_difference(out[s, :n + 1], want)
                assert (out[s, n + 1:] == M.GUARD_WORD).all(), tag + ": a store behind out[n]"
                if form == 1:
                    assert first_difference(aux[s, :nb], np.uint64(M.PFX) | with_tail, False) is None, tag + ": " + first_difference(aux[s, :nb], np.uint64(M.PFX) | with_tail, False)
                    assert (aux[s, nb:] == GUARD64).all(), tag + ": a store behind desc[nb - 1]"
                else:
                    assert (aux[s, M.tmp_words(n):] == M.GUARD_WORD).all(), tag + ": a store behind tmp's 2 (nb + 1) + 2 (nb2 + 1) words"
                    if nb == 1:
                        assert (aux[s] == M.GUARD_WORD).all(), tag + ": one block touches no tmp"
                answers.append(out[s, :n + 1])
    for o in answers[1:]:
        assert np.array_equal(o, answers[0]), what + ": the forms, streams and values of in[n] do not agree"


def scan_cases():
    for n in sorted(M.SCAN_SIZES):
        for pattern in M.patterns_for(n):
            if pattern == "step":
                for p in M.STEP_AT:
                    if p < n:
                        yield pytest.param(n, pattern, p, id="%d-step%d" % (n, p))
            else:
                yield pytest.param(n, pattern, None, id="%d-%s" % (n, pattern))


@pytest.mark.parametrize("n,pattern,step_at", list(scan_cases()))
def test_scan_both_forms_against_cumsum(L, n, pattern, step_at):
    check_scan(L, M.make(pattern, n, 0, seed=n % 1000 + 1, step_at=step_at), what="n = %d, %s" % (n, pattern))


@pytest.fixture(scope="module")
def own_grid(L):
    return run_scan(L, 1, np.zeros(1, np.uint32))[2]


@pytest.mark.parametrize("seeded", [0, 1])
@pytest.mark.parametrize("cap", M.GRID_CAPS)
def test_one_launch_scan_at_a_capped_grid(L, own_grid, cap, seeded):
    """Workgroup 0 takes one, two and three blocks, the last of them partial: the grid-stride loop, and the barrier at its head that keeps sh / sh_excl of the block before."""
    grid = run_scan(L, 1, np.zeros(1, np.uint32), grid_cap=cap)[2]
    assert 16 <= own_grid <= 1024 and grid == (min(cap, own_grid) if cap else own_grid), "the cap never raises the grid"
    for nb, most in zip(M.capped_blocks(grid), ([1] if grid > 1 else []) + [1, 2, 3]):
        n = M.n_for_blocks(nb)
        assert M.levels(n)[0] == nb and max(M.iterations(nb, grid)) == most
        for pattern in ("ones", "random"):
            check_scan(L, M.make(pattern, n, 0, seed=nb), forms=(1,), grid_cap=cap, seeded=seeded, what="grid %d, %d blocks, %s, seeded %d" % (grid, nb, pattern, seeded))


@pytest.mark.parametrize("seeded", [0, 1])
@pytest.mark.parametrize("nb", M.OWN_GRID_BLOCKS)
def test_one_launch_scan_over_more_than_a_window_of_predecessors(L, nb, seeded):
    n = M.n_for_blocks(nb)
    for pattern in ("ones", "wrap", "random"):
        check_scan(L, M.make(pattern, n, 0, seed=nb), seeded=seeded, what="%d blocks, %s, seeded %d" % (nb, pattern, seeded))


@pytest.mark.parametrize("blocks,seeded", [(17, 0), (300, 0), (300, 1), (4097, 0), (None, 0), (None, 1)])
def test_two_one_launch_scans_at_once(L, own_grid, blocks, seeded):
    """A build's front and main stream: two scans, each at the launcher's own grid (agx_scan_grid halves what the device holds for this).  None: workgroup 0 of both takes three blocks."""
    nb = blocks if blocks else 2 * own_grid + 1
    n = M.n_for_blocks(nb)
    check_scan(L, M.make("random", n, 0, seed=nb), forms=(1,), seeded=seeded, streams=2, what="two streams, %d blocks, seeded %d" % (nb, seeded))


# ---- agx_k_zero -----------------------------------------------------------------------------------------------------------------------------------------------------
ZERO_CASES = [
    (0, 0, 0, 0, 0, 0, 0, 0),                                       # no launch
    (1, 0, 0, 0, 0, 0, 0, 0),
    (0, 0, 0, 0, 0, 0, 0, 1),
    (255, 1, 0, 256, 257, 0, 3, 4096),
    (256, 512, 768, 1024, 256, 1280, 2560, 256),
    (1048577, 0, 1, 255, 0, 4097, 0, 1),
]


@pytest.mark.parametrize("lens", ZERO_CASES, ids=lambda t: "-".join(map(str, t)))
def test_zero_clears_its_eight_segments_and_nothing_else(L, lens):
    words = np.full(sum(lens) + 16 * G, 0x12345678, np.uint32)
    assert L.agx_test_zero(0, (ctypes.c_uint32 * 8)(*lens), words.ctypes.data_as(U32)) == 0
    at = 0
    for s, n in enumerate(lens):
        front, body, back = words[at:at + G], words[at + G:at + G + n], words[at + G + n:at + 2 * G + n]
        assert (front == M.GUARD_WORD).all(), "segment %d: a store in front of it" % s
        bad = np.flatnonzero(body)
        assert not len(bad), "segment %d: %d of %d words not cleared, the first at %d" % (s, len(bad), n, bad[0] if len(bad) else -1)
        assert (back == M.GUARD_WORD).all(), "segment %d: a store behind it" % s
        at += n + 2 * G
    assert at == len(words)


# ---- agx_k_copy_out ---------------------------------------------------------------------------------------------------------------------------------------------------
COPY_CASES = [
    (0,), (16,), (4080,), (4096,), (4112,), (1600000,),
    (16, 4080, 4096, 4112),
    (4096, 0, 4112, 16, 1600000),                                   # the second launch holds a single live segment
    (1, 15, 17, 4080, 4095, 4097, 0, 1600000),                      # byte counts that are rounded up to 16
    (16, 0, 4096, 4112, 4080, 1600000, 16, 0, 33),                  # a zero-length segment between two live ones; a third launch
    (0, 0, 0, 0, 4112),                                             # a launch with nothing in it is not made
    (16777216 + 4112,),                                             # more 16-byte words than 512 blocks x 256 threads x 8: the grid's upper limit
]


@pytest.mark.parametrize("sizes", COPY_CASES, ids=lambda t: "-".join(map(str, t)))
def test_copy_out_copies_its_segments_and_nothing_else(L, sizes):
    rounded = [(b + 15) // 16 * 16 for b in sizes]
    src = np.frombuffer(np.random.RandomState(len(sizes)).bytes(max(sum(rounded), 1)), np.uint8).copy()
    dst = np.zeros(sum(rounded) + len(sizes) * 4 * G, np.uint8)
    assert L.agx_test_copy_out(0, len(sizes), (ctypes.c_uint64 * len(sizes))(*sizes), src.ctypes.data_as(U8), dst.ctypes.data_as(U8)) == 0
    at = frm = 0
    for s, r in enumerate(rounded):
        bad = np.flatnonzero(dst[at:at + r] != src[frm:frm + r])
        assert not len(bad), "segment %d of %s: %d bytes differ, the first at %d" % (s, sizes, len(bad), bad[0] if len(bad) else -1)
        assert (dst[at + r:at + r + 4 * G] == 0xA5).all(), "segment %d of %s: a store behind its rounded-up end" % (s, sizes)
        at += r + 4 * G
        frm += r
    assert at == len(dst)
