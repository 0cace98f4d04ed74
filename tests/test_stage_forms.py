"""The upload forms of a unit's read alignments (aligngraph_amd/csrc/agx_forms.h) on the CPU: the functions the engine's staging calls, over numpy arrays, through
tests/wire_shim.cpp (tests/forms_shim.py builds it).

  * the tile-ordered gather against a numpy model written from the definitions of agx_core.h ("hits in tile order": agx_whit_first_x; AGX_WF_DUP: agx_idx0_pos and
    agx_hit_dup_by on the wire forms), on the staged arrays of small hand-made units (tests/front_units.py), with the hits packed inside it;
  * the hit packer across thread counts and block edges, and the two ways its finish says "no gain";
  * the window cuts and a window's piece of the rows on made-up tile_first arrays.
Every comparison is an equality of integers or bytes.  Nothing here needs a device."""
import ctypes
import os

import numpy as np
import pytest

import damaged_inputs as D
import forms_shim as FS
import front_units as FU
from hostsim import sim
from lean_units import K, Unit
from forms_shim import BLOCK, WHIT, plain_hits

L = 100                      # read length: a packed row of 25 bytes, no multiple of 16
NONE = 0xFFFFFFFF
THREADS = (1, 2, 5)          # (five: thread edges on whole blocks that are not the halves)
SIZES = (1, 63, 64, 65, 129)      # hits: the packer's block edges


# ---- the units ----------------------------------------------------------------------------------------------------------------------------

def unit_of(nh):
    """A unit of nh hits.  From eight hits on: a pair whose second hit lands within a read length of its first (a duplicate) and one whose second hit does not; a pair with a
    second hit whose mate 1 is clipped in front (its first run does not start at read index 0); a pair whose row lists its first and its last base.  Left mates scattered
    over the tiles, so that the tile order is not the file order."""
    special = 3 if nh >= 8 else 0
    n_pairs = nh - special
    place = lambda i: 150 + ((i * 37) % max(n_pairs, 1)) * 13      # noqa: E731
    pairs = [FU.P(place(i), L) for i in range(n_pairs)]
    more = {}
    if special:
        more = {0: [(place(0) + 30, place(0) + 430)], 1: [(place(1) + 700, place(1) + 1100)], 2: [(place(2) + 20, place(2) + 420)]}
        pairs[2] = FU.P(place(2), L, cigar="5S95M")
        pairs[3] = FU.P(place(3), L, bases={0: "N", L - 1: "N"})
    return FU.Case("forms%d" % nh, "forms", Unit(4096, pairs), L, [], more=more)


class Staged:
    """The staged arrays of a unit as the loaders make them (tmp/_agx_pairs.<u>.bin written from the text), and the tile order by the model."""

    def __init__(self, nh, run):
        tmp = FU.write_unit(unit_of(nh), run)
        path, msg = os.path.join(run, "_agx_pairs.0.bin"), ctypes.create_string_buffer(512)
        lib = sim._lib_now()
        lib.agx_hostsim_write_pairs_file.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        assert lib.agx_hostsim_write_pairs_file(tmp.encode(), 0, K, 1000000, 2, path.encode(), msg, 512) == 0, msg.value
        d = D.PairsDoor(path, 4096, run)
        self.hits, self.sides, self.runs = (np.ascontiguousarray(d.a[s]) for s in ("hits", "sides", "runs"))
        self.other, self.codes = np.ascontiguousarray(d.a["other"]), np.ascontiguousarray(d.a["codes"])
        self.nh, self.n_rows, self.stride, self.maxlen = d.n["nh"], d.n["n_rows"], d.n["stride"], d.n["maxlen"]
        assert self.nh == nh and self.stride == L and (self.stride // 4) % 16 != 0
        self.perm = np.argsort(self.first_x() // 64, kind="stable").astype(np.uint32)      # hit numbers ascend inside a tile

    def left_first_x(self, w):      # agx_whit_first_x
        f = int(w["flags"])
        if not f & (D.RUNS2 if f & D.LEFT2 else D.RUNS1):
            return int(w["b"] if f & D.LEFT2 else w["a"])
        sd = self.sides[int(w["a"] if f & D.RUNS1 else w["b"])]
        first, n = (int(sd["runs2"]), int(sd["nruns"]) >> 16) if f & D.LEFT2 else (int(sd["runs1"]), int(sd["nruns"]) & 0xFFFF)
        return next((int(r["t"]) for r in self.runs[first:first + n] if r["n"]), 0)

    def first_x(self):
        return np.array([self.left_first_x(w) for w in self.hits], np.int64)

    def idx0(self, w):      # agx_idx0_pos on the wire forms: positionSets[hit][0] of mate 1
        if not w["flags"] & D.RUNS1:
            return int(w["a"])
        r = self.runs[int(self.sides[int(w["a"])]["runs1"])]
        return int(r["t"]) if r["q"] == 0 else NONE

    def dup(self, h):      # agx_hit_dup_by
        w, me = self.hits[h], self.idx0(self.hits[h])

        def absdiff(a, b):
            d = (a - b) & 0xFFFFFFFF
            return abs(d - (1 << 32) if d >= 1 << 31 else d)
        return any(absdiff(me, self.idx0(self.hits[h - e])) < int(w["len"]) for e in range(1, int(w["back"]) + 1))


@pytest.fixture(scope="module")
def staged(built, tmp_path_factory):
    made = {}

    def get(nh):
        if nh not in made:
            made[nh] = Staged(nh, str(tmp_path_factory.mktemp("forms%d" % nh)))
        return made[nh]
    return get


def gather(S, threads, compact=1):
    nh, s4 = S.nh, S.stride // 4
    cap = 8 * len(S.other) + 16
    c = np.array([nh, len(S.sides), len(S.runs), len(S.other), S.n_rows, S.stride, S.maxlen, cap], np.uint64)
    wire, hits_t, codes_t, slot_row = np.zeros((nh + 1) * 16, np.uint8), np.zeros(nh + 1, WHIT), np.full(nh * s4 + 16, 0xEE, np.uint8), np.zeros(nh, np.uint32)
    other_t, out = np.zeros(cap, np.uint64), np.zeros(7, np.uint64)
    hits_t[nh] = (7, 7, 7, 7, 7, 7)
    n = FS.lib().agx_forms_gather(c.ctypes.data, S.hits.ctypes.data, S.sides.ctypes.data, S.runs.ctypes.data, S.other.ctypes.data, S.codes.ctypes.data, S.perm.ctypes.data, threads, compact,
                                  wire.ctypes.data, hits_t.ctypes.data, codes_t.ctypes.data, slot_row.ctypes.data, other_t.ctypes.data, out.ctypes.data)
    assert n <= cap
    assert tuple(hits_t[nh]) == (7, 7, 7, 7, 7, 7) and (codes_t[nh * s4:] == 0xEE).all(), "a write behind the last record or the last row"
    return dict(hits_t=hits_t[:nh], codes_t=codes_t[:nh * s4], slot_row=slot_row, other_t=other_t[:n], wire=wire, out=[int(x) for x in out])


# ---- the gather ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nh", SIZES)
def test_gather_is_the_model(staged, nh):
    S = staged(nh)
    g, s4 = gather(S, 1), S.stride // 4
    dups = 0
    for i, h in enumerate(S.perm.tolist()):
        w, t = S.hits[h], g["hits_t"][i]
        row = int(w["row"])
        want_flags = int(w["flags"]) | (D.DUP if S.dup(h) else 0)
        dups += bool(want_flags & D.DUP)
        assert (int(t["a"]), int(t["b"]), int(t["len"]), int(t["back"])) == (int(w["a"]), int(w["b"]), int(w["len"]), int(w["back"])), i
        assert int(t["row"]) == h and int(t["flags"]) == want_flags, (i, h)
        assert g["codes_t"][i * s4:(i + 1) * s4].tobytes() == S.codes[row * s4:(row + 1) * s4].tobytes(), i
        assert int(g["slot_row"][i]) == row
    want_other = [i * S.stride + int(e) % S.stride for i, h in enumerate(S.perm.tolist()) for e in S.other if int(e) // S.stride == int(S.hits[h]["row"])]
    assert g["other_t"].tolist() == want_other and want_other == sorted(set(want_other))
    if nh >= 8:      # the unit has what it was made for
        h = S.hits
        assert dups >= 1 and any(int(w["back"]) and not S.dup(i) for i, w in enumerate(h)), "a second hit that is a duplicate, and one that is not"
        assert any(int(w["back"]) and (w["flags"] & D.RUNS1) and S.runs[int(S.sides[int(w["a"])]["runs1"])]["q"] != 0 for w in h), "a later hit whose mate 1 does not begin at read index 0"
        firsts = set(int(e) % S.stride for e in S.other)
        assert 0 in firsts and L - 1 in firsts, "a row whose first and last bases are listed"
        assert not np.array_equal(S.perm, np.arange(nh)), "the tile order is not the file order"


@pytest.mark.parametrize("nh", SIZES)
def test_gather_is_the_same_bytes_on_any_number_of_threads(staged, nh):
    S = staged(nh)
    one = gather(S, 1)
    bytes_used = 0
    if one["out"][1]:      # the blocks gained: blocks, escapes, extra words lie behind one another in the wire buffer
        n_blocks, ne, nx, e_at, x_at = one["out"][2:7]
        assert n_blocks == (nh + 63) // 64 and e_at == n_blocks * BLOCK.itemsize and x_at == e_at + ne * 16
        bytes_used = x_at + nx * 4
        # the blocks made inside the gather are the blocks made over the finished array
        blocks, esc, ext, counts = np.zeros(n_blocks, BLOCK), np.zeros(nh + 1, WHIT), np.zeros(nh + 1, np.uint32), np.zeros(2, np.uint32)
        FS.lib().agx_wire_pack_hits(np.ascontiguousarray(one["hits_t"]).ctypes.data, nh, S.maxlen, 1, blocks.ctypes.data, esc.ctypes.data, ext.ctypes.data, counts.ctypes.data)
        assert (int(counts[0]), int(counts[1])) == (ne, nx)
        assert one["wire"][:bytes_used].tobytes() == blocks.tobytes() + esc[:ne].tobytes() + ext[:nx].tobytes()
    for threads in THREADS[1:]:
        g = gather(S, threads)
        assert g["out"] == one["out"]
        for key in ("hits_t", "codes_t", "slot_row", "other_t"):
            assert g[key].tobytes() == one[key].tobytes(), (key, threads)
        assert g["wire"][:bytes_used].tobytes() == one["wire"][:bytes_used].tobytes(), threads
    plain = gather(S, 2, compact=0)      # (AGX_WIRE_PLAIN: the same forms, no blocks)
    assert plain["out"][:2] == [0, 0] and all(plain[key].tobytes() == one[key].tobytes() for key in ("hits_t", "codes_t", "slot_row", "other_t"))


def test_the_larger_units_pack_their_hits_inside_the_gather(staged):
    """The packer is on where the blocks alone are fewer bytes than the records: not for one hit, nor for 65 (two blocks of 528 bytes against 65 records of 16)."""
    assert [bool(gather(staged(nh), 2)["out"][0]) for nh in SIZES] == [((nh + 63) // 64) * BLOCK.itemsize < nh * 16 for nh in SIZES] == [False, True, True, False, True]
    assert gather(staged(129), 2)["out"][1] == 1


# ---- the packer ---------------------------------------------------------------------------------------------------------------------------

def packed(hits, threads, maxlen=150):
    n = len(hits)
    blocks, esc, ext, counts = np.zeros((n + 63) // 64, BLOCK), np.zeros(n + 1, WHIT), np.zeros(n + 1, np.uint32), np.zeros(2, np.uint32)
    FS.lib().agx_wire_pack_hits(hits.ctypes.data, n, maxlen, threads, blocks.ctypes.data, esc.ctypes.data, ext.ctypes.data, counts.ctypes.data)
    return blocks.tobytes(), esc[:int(counts[0])].tobytes(), ext[:int(counts[1])].tobytes()


def pack_wire(hits, threads, maxlen=150):
    n = len(hits)
    wire, out = np.zeros((n + 1) * 16, np.uint8), np.zeros(7, np.uint64)
    FS.lib().agx_forms_pack_wire(hits.ctypes.data, n, maxlen, threads, wire.ctypes.data, out.ctypes.data)
    return wire, [int(x) for x in out]


@pytest.mark.parametrize("n", SIZES + (5000,))
def test_packer_is_the_same_bytes_on_any_number_of_threads(n):
    h = plain_hits(n, seed=n)
    h["back"][::7] = 1      # escapes in every block
    one = packed(h, 1)
    assert len(one[1]) == 16 * len(h[::7]) and len(one[0]) == BLOCK.itemsize * ((n + 63) // 64)
    for threads in THREADS[1:]:
        assert packed(h, threads) == one, threads
    wire, out = pack_wire(h, 5)
    if out[1]:      # where the blocks gain, the engine's buffer holds the three behind one another
        assert out[2:5] == [(n + 63) // 64, len(one[1]) // 16, len(one[2]) // 4] and out[5] == len(one[0]) and out[6] == out[5] + len(one[1])
        assert wire[:out[6] + len(one[2])].tobytes() == b"".join(one)
    on = len(one[0]) < n * 16
    assert (bool(out[0]), bool(out[1])) == (on, on and sum(len(x) for x in one) < n * 16)


def test_finish_says_no_gain():
    # a few dozen records: the last block's empty slots outweigh the rest — the packer is not even on
    for n in (1, 30, 33):
        assert pack_wire(plain_hits(n), 2)[1][:2] == [0, 0], n
    # 34: the one block is 16 bytes fewer than the records, and the extra words of the hits with side records take more than that
    h = plain_hits(34)
    assert len(packed(h, 2)[2]) > 16 and pack_wire(h, 2)[1][:5] == [1, 0, 1, 0, len(packed(h, 2)[2]) // 4]
    assert pack_wire(plain_hits(60), 2)[1][:2] == [1, 1]
    # every record escapes: the blocks and the records they could not hold are more bytes than the records
    h = plain_hits(5000)
    h["back"] = 1
    out = pack_wire(h, 2)[1]
    assert out[:5] == [1, 0, (5000 + 63) // 64, 5000, 0] and out[5:] == [0, 0]
    assert pack_wire(plain_hits(5000), 2)[1][:2] == [1, 1]


# ---- the cuts and the pieces --------------------------------------------------------------------------------------------------------------

def model_cuts(n_pos, n_tiles, forced):
    W = max(1, min(forced if forced else n_pos // 8000000, 8, n_tiles))
    return W, [n_tiles * w // W for w in range(W + 1)]


@pytest.mark.parametrize("forced", [0, 1, 2, 3, 8, 9, 1000])
@pytest.mark.parametrize("n_pos", [1, 64, 65, 130, 4096, 70001, 7999999, 8000000, 24000001, 80000000])
def test_window_cuts(n_pos, forced):
    n_tiles = (n_pos + 63) // 64
    assert FS.window_cuts(n_pos, n_tiles, forced) == model_cuts(n_pos, n_tiles, forced)


def tile_first_of(nh, n_tiles, seed):
    """hits in front of every tile's own: ascending, n_tiles + 2 entries, the last two = nh (order_hits)"""
    rnd = np.random.RandomState(seed)
    return np.concatenate((np.sort(rnd.randint(0, nh + 1, n_tiles)) * (np.arange(n_tiles) > 0), [nh, nh])).astype(np.uint32)


PIECE_UNITS = [("many", 1000, 40, 1), ("few hits: an early window reaches the last row", 20, 8, 2), ("one hit", 1, 8, 3), ("rows in the last tile only", 300, 12, 4), ("two tiles", 200, 2, 5)]


@pytest.mark.parametrize("diffed", [False, True], ids=["two_bit", "row_diff"])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("name,nh,n_tiles,seed", PIECE_UNITS, ids=[u[0].split(":")[0].replace(" ", "_") for u in PIECE_UNITS])
def test_pieces_partition_the_rows(name, nh, n_tiles, seed, W, diffed):
    stride, s4 = 100, 25
    tf = tile_first_of(nh, n_tiles, seed)
    if name.startswith("few"):
        tf[:n_tiles] = [0, 3, 5, 10, 12, 18, 19, 19]      # W = 3 cuts at tiles 2 and 5: window 1 begins at row 16 and holds the last row, window 2 is empty
    if name.startswith("rows in the last"):
        tf[:n_tiles] = 0
    n_win, cuts = FS.window_cuts(n_tiles * 64, n_tiles, W)
    assert n_win == min(W, n_tiles)
    rnd = np.random.RandomState(seed)
    other_t = np.unique(np.concatenate((rnd.randint(0, nh * stride, 50), [0, nh * stride - 1]))).astype(np.uint64)      # (the first and the last base of all among them)
    n_blocks = (nh + 63) // 64
    block_off = np.arange(n_blocks + 1, dtype=np.uint32) * 7 if diffed else None
    n_rowcnt = n_blocks * 64 + 64
    align = 64 if diffed else 16
    pieces = [FS.row_piece(nh, stride, cuts, tf, other_t, w, w + 1, block_off, n_rowcnt) for w in range(n_win)]
    assert pieces[0]["r_lo"] == 0 and pieces[-1]["r_hi"] == nh
    holders = 0
    for w, p in enumerate(pieces):
        assert p["r_lo"] <= p["r_hi"] and (w == 0 or p["r_lo"] == pieces[w - 1]["r_hi"])
        assert p["r_hi"] == nh or p["r_hi"] % align == 0
        assert p["r_hi"] == nh or p["r_hi"] == min(nh, (int(tf[cuts[w + 1]]) + align - 1) // align * align), "a window begins at the first hit of its first tile, rounded up"
        assert other_t[p["o_lo"]:p["o_hi"]].tolist() == [int(e) for e in other_t if p["r_lo"] <= int(e) // stride < p["r_hi"]]
        if diffed:
            assert (p["blk_lo"], p["blk_hi"], p["cnt_lo"], p["cnt_hi"]) == (p["r_lo"] // 64, (p["r_hi"] + 63) // 64, p["r_lo"], (p["r_hi"] + 63) // 64 * 64)
            assert (p["unit_lo"], p["unit_hi"]) == (7 * p["blk_lo"], 7 * p["blk_hi"]) and (p["code_lo"], p["code_hi"]) == (0, 0)
        else:
            assert (p["code_lo"], p["code_hi"]) == (p["r_lo"] * s4, p["r_hi"] * s4)
        if p["r_hi"] == p["r_lo"]:
            continue      # a window without rows: nothing is copied or expanded for it
        assert p["v_lo"] == p["r_lo"] * stride
        if p["r_hi"] == nh:      # the piece that holds the last row is padded like the whole array
            holders += 1
            assert p["v_hi"] == (nh * stride + 15) // 16 * 16
        else:
            assert p["v_hi"] == p["r_hi"] * stride and p["v_hi"] % 16 == 0
    assert holders == 1
    whole = FS.row_piece(nh, stride, cuts, tf, other_t, 0, n_win, block_off, n_rowcnt)
    assert (whole["r_lo"], whole["r_hi"], whole["o_lo"], whole["o_hi"], whole["v_hi"]) == (0, nh, 0, len(other_t), (nh * stride + 15) // 16 * 16)


def test_the_fuzz_case_reaches_the_last_row_early():
    """r06's fuzz: few hits, three windows — the second piece holds the last row and is the padded one, the third is empty."""
    nh, stride = 20, 100
    tf = np.array([0, 3, 5, 10, 12, 18, 19, 19, nh, nh], np.uint32)
    n_win, cuts = FS.window_cuts(512, 8, 3)
    assert (n_win, cuts) == (3, [0, 2, 5, 8])
    p = [FS.row_piece(nh, stride, cuts, tf, np.zeros(0, np.uint64), w, w + 1) for w in range(3)]
    assert [(x["r_lo"], x["r_hi"]) for x in p] == [(0, 16), (16, 20), (20, 20)]
    assert (p[0]["v_lo"], p[0]["v_hi"]) == (0, 1600) and (p[1]["v_lo"], p[1]["v_hi"]) == (1600, 2000) and 2000 % 16 == 0
    nh = 19      # (a last row that does not end on a group of 16 bases)
    tf[8:] = nh
    tf[5:8] = 18
    p = [FS.row_piece(nh, stride, cuts, tf, np.zeros(0, np.uint64), w, w + 1) for w in range(3)]
    assert [(x["r_lo"], x["r_hi"]) for x in p] == [(0, 16), (16, 19), (19, 19)] and (p[1]["v_lo"], p[1]["v_hi"]) == (1600, 1904)


def test_more_windows_than_tiles():
    assert FS.window_cuts(100, 2, 8) == (2, [0, 1, 2])
    tf = np.array([0, 40, 70, 70], np.uint32)
    p = [FS.row_piece(70, 100, [0, 1, 2], tf, np.zeros(0, np.uint64), w, w + 1) for w in range(2)]
    assert [(x["r_lo"], x["r_hi"]) for x in p] == [(0, 48), (48, 70)]
