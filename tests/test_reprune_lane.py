"""agx_reprune_lane (csrc/agx_core.h), the lane function of agx_unit_reprune's kernel, on the CPU: tests/reprune_shim.cpp runs it serially, tile by tile, over
plain arrays (lane = position, the in-tile prefix in plain C), and numpy says what must come out.  The tables are the oracle's graph dumps of two generated units
(seed 201: the last tile is partial; seed 203: many variants at most positions, ten side ids per position) and of the pile-up unit (180 variants at every position of a pile: the
in-tile prefix passes 63 x 179).  Flags start as the build's at the unit's own coverage with random CONTIG / EOVF bits; the thresholds are applied in turn to the
same flag bytes, as a sweep over a resident unit does.  tests/test_gpu_reprune.py runs the kernel itself."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import harness as H
import walk_model as WM
from conftest import write_pileup_unit
from test_gpu_parity import CONFIGS

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "reprune_shim.cpp")
NONE = 0xFFFFFFFF
DEAD, CONTIG, EOVF = 1, 2, 4      # AGX_NF_* (agx_core.h)
TILE = 64
THRESHOLDS = (0, 1, 3, 5, 8, 20, 1 << 30)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("reprune_shim") / "libreprune_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, SHIM])
    L = ctypes.CDLL(so)
    P = ctypes.POINTER
    L.agx_reprune_shim.argtypes = [P(ctypes.c_uint32), P(ctypes.c_uint16), P(ctypes.c_uint32), P(ctypes.c_int), P(ctypes.c_uint8), ctypes.c_uint32, ctypes.c_uint32,
                                   ctypes.c_uint32, P(ctypes.c_uint32), P(ctypes.c_uint32)]
    return L


def _synth(tmp_path_factory, seed):
    cfg = next(c for c in CONFIGS if c["seed"] == seed)
    run = H.synth(str(tmp_path_factory.mktemp("run%d" % seed) / "run"), sam_seq=0, **cfg)
    meta = H.read_meta(run)
    return os.path.join(run, "tmp"), meta["k"], meta["insert_variation"], meta["coverage"]


def _pileup(tmp_path_factory):
    return write_pileup_unit(str(tmp_path_factory.mktemp("pileup")), 180, spacing=300), 5, 50, 3


UNITS = {"seed201": lambda f: _synth(f, 201), "seed203": lambda f: _synth(f, 203), "pileup180": _pileup}


@pytest.fixture(scope="module")
def graph_of(built, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            tmp, k, iv, cov = UNITS[name](tmp_path_factory)
            made[name] = (H.run_oracle(tmp, 0, k, iv, cov, graph=True)["graph"], cov)
        return made[name]
    return get


def ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


@pytest.mark.parametrize("name", list(UNITS))
def test_lane_function_matches_numpy_at_every_threshold(shim, graph_of, name):
    g, cov0 = graph_of(name)
    n_pos, nn = int(g["n_pos"]), int(g["n_nodes"])
    ns = g["node_start"].astype(np.int64)
    per_pos = np.diff(ns)
    if name == "seed201":
        assert n_pos % TILE, "the last tile must be partial"
    if name == "seed203":
        assert per_pos.max() > 4 and nn > 5 * n_pos, "many variants per position: more side ids than positions"
    if name == "pileup180":
        assert (per_pos[: n_pos // TILE * TILE].reshape(-1, TILE) >= 180).all(axis=1).any(), "a whole tile of 180-variant positions"
    pos_of = np.repeat(np.arange(n_pos, dtype=np.int64), per_pos)
    cid = np.ascontiguousarray(g["node_key"][:, 0], dtype=np.uint32)
    coff = g["node_key"][:, 1]
    counts = np.ascontiguousarray(g["node_cnt"], dtype=np.int32)
    node_start = np.ascontiguousarray(g["node_start"][:n_pos], dtype=np.uint32)
    node_cnt = np.ascontiguousarray(per_pos, dtype=np.uint16)
    rnd = np.random.RandomState(7)
    other = (np.where(coff != NONE, CONTIG, 0) | (rnd.randint(0, 2, nn) * CONTIG) | (rnd.randint(0, 2, nn) * EOVF) | (rnd.randint(0, 2, nn) * 0xF8)).astype(np.uint8)
    flags = (other | np.where((cid == NONE) & (counts[:, 0] < cov0), DEAD, 0)).astype(np.uint8)
    n_tiles = (n_pos + TILE - 1) // TILE
    side_pk, tile_side = np.full(n_pos, 0xDEADBEEF, np.uint32), np.full(n_tiles, 0xDEADBEEF, np.uint32)
    for c in THRESHOLDS:
        rc = shim.agx_reprune_shim(ptr(node_start, ctypes.c_uint32), ptr(node_cnt, ctypes.c_uint16), ptr(cid, ctypes.c_uint32), ptr(counts, ctypes.c_int),
                                   ptr(flags, ctypes.c_uint8), n_pos, nn, c, ptr(side_pk, ctypes.c_uint32), ptr(tile_side, ctypes.c_uint32))
        assert rc == 0
        dead = (cid == NONE) & (counts[:, 0].astype(np.int64) < c)
        assert np.array_equal((flags & DEAD) != 0, dead), c
        assert np.array_equal(flags & ~np.uint8(DEAD), other), c
        alive_at = np.bincount(pos_of[~dead], minlength=n_pos)
        side = np.maximum(alive_at - 1, 0)
        padded = np.zeros(n_tiles * TILE, np.int64)
        padded[:n_pos] = side
        tiles = padded.reshape(n_tiles, TILE)
        before = (np.cumsum(tiles, axis=1) - tiles).reshape(-1)[:n_pos]
        assert before.max() < 65536
        assert np.array_equal(side_pk, (before | (side << 16)).astype(np.uint32)), c
        assert np.array_equal(tile_side, tiles.sum(axis=1).astype(np.uint32)), c
        assert int(tile_side.sum()) == WM.build(g, c)["n_ids"] - n_pos, c


def test_in_tile_prefix_passes_63_times_179(shim, graph_of):
    """The pile-up unit at threshold 0: every variant alive, the prefix in front of a pile tile's last position is 63 x 179."""
    g, _ = graph_of("pileup180")
    n_pos, nn = int(g["n_pos"]), int(g["n_nodes"])
    per_pos = np.diff(g["node_start"].astype(np.int64))
    cid = np.ascontiguousarray(g["node_key"][:, 0], dtype=np.uint32)
    counts = np.ascontiguousarray(g["node_cnt"], dtype=np.int32)
    node_start = np.ascontiguousarray(g["node_start"][:n_pos], dtype=np.uint32)
    node_cnt = np.ascontiguousarray(per_pos, dtype=np.uint16)
    flags = np.zeros(nn, np.uint8)
    n_tiles = (n_pos + TILE - 1) // TILE
    side_pk, tile_side = np.zeros(n_pos, np.uint32), np.zeros(n_tiles, np.uint32)
    assert shim.agx_reprune_shim(ptr(node_start, ctypes.c_uint32), ptr(node_cnt, ctypes.c_uint16), ptr(cid, ctypes.c_uint32), ptr(counts, ctypes.c_int),
                                 ptr(flags, ctypes.c_uint8), n_pos, nn, 0, ptr(side_pk, ctypes.c_uint32), ptr(tile_side, ctypes.c_uint32)) == 0
    assert not flags.any()
    assert (side_pk & 0xFFFF).max() >= 63 * 179 and tile_side.max() >= 64 * 179


def test_threshold_above_the_signed_range_is_refused(shim):
    z32, z16, zi, z8 = np.zeros(1, np.uint32), np.zeros(1, np.uint16), np.zeros(6, np.int32), np.zeros(1, np.uint8)
    assert shim.agx_reprune_shim(ptr(z32, ctypes.c_uint32), ptr(z16, ctypes.c_uint16), ptr(z32, ctypes.c_uint32), ptr(zi, ctypes.c_int), ptr(z8, ctypes.c_uint8), 1, 1, 1 << 31,
                                 ptr(z32.copy(), ctypes.c_uint32), ptr(z32.copy(), ctypes.c_uint32)) == -1
