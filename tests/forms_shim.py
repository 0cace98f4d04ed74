"""tests/wire_shim.cpp as a shared library, built once per process: the product's upload forms (aligngraph_amd/csrc/agx_forms.h) over numpy arrays, for the CPU tests that
call them (tests/test_wire_codec.py, tests/test_stage_forms.py, the window cuts in tests/test_sweep_cases.py), with the record types and the hits those tests share.  The
shim is compiled alone, by g++ with -Wall -Wextra -Werror."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P, U32, U64, INT = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
WHIT = np.dtype([("a", "<u4"), ("b", "<u4"), ("row", "<u4"), ("len", "<u2"), ("flags", "u1"), ("back", "u1")])      # agx_whit
WSIDE = np.dtype([("runs1", "<u4"), ("runs2", "<u4"), ("nruns", "<u4")])                                           # agx_wside
BLOCK = np.dtype([("base", "<u4"), ("esc", "<u4"), ("ext", "<u4"), ("pad", "<u4"), ("num", "<u4", 64), ("word", "<u4", 64)])      # agx_chit_block
LISTED = np.dtype([("side", "<u4"), ("nruns", "<u4")])                                                             # agx_cside_esc
REV1, REV2, LEFT2, RUNS1, RUNS2, DUP = 1, 2, 4, 8, 16, 32
L = 150      # the unit's longest read in most cases
PIECE_FIELDS =("r_lo", "r_hi", "code_lo", "code_hi", "cnt_lo", "cnt_hi", "blk_lo", "blk_hi", "unit_lo", "unit_hi", "v_lo", "v_hi", "o_lo", "o_hi")      # RowPiece


@functools.lru_cache(maxsize=None)
def lib():
    d = tempfile.mkdtemp(prefix="agx_forms_shim_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libforms_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "wire_shim.cpp")])
    L = ctypes.CDLL(so)
    L.agx_wire_pack_hits.argtypes = [P, U32, U32, U32, P, P, P, P]
    L.agx_wire_unpack_hits.argtypes = L.agx_wire_unpack_hits_serial.argtypes = [P, U32, U32, P, P, P]
    L.agx_wire_pack_sides.argtypes = [P, U32, P, P, P, P]
    L.agx_wire_unpack_sides.argtypes = [P, U32, P, U32, U32, P]
    L.agx_forms_pack_wire.argtypes = [P, U32, U32, U32, P, P]
    L.agx_forms_gather.argtypes = [P, P, P, P, P, P, P, U32, INT, P, P, P, P, P, P]
    L.agx_forms_gather.restype = U64
    L.agx_forms_window_cuts.argtypes = [U64, U64, U32, P]
    L.agx_forms_window_cuts.restype = U32
    L.agx_forms_row_piece.argtypes = [P, P, P, INT, P, P, U32, U32, P]
    return L


def plain_hits(n, seed=1, start=50000):
    """n hits as the loaders make them in tile order: positions that grow slowly, the other mate an insert size away, some with a side record."""
    rnd = np.random.RandomState(seed)
    h = np.zeros(n, WHIT)
    at = start + np.cumsum(rnd.randint(0, 12, n)).astype(np.uint32)
    flags = rnd.randint(0, 4, n) | (rnd.randint(0, 2, n) * DUP)
    kind = rnd.randint(0, 8, n)      # 0: mate 1 has runs, 1: mate 2, 2: both
    flags = flags | np.where(kind == 0, RUNS1, 0) | np.where(kind == 1, RUNS2, 0) | np.where(kind == 2, RUNS1 | RUNS2, 0)
    side = rnd.randint(0, 1 << 31, n).astype(np.uint32)
    other = at + 350 + rnd.randint(-40, 40, n).astype(np.uint32)
    h["a"] = np.where(flags & RUNS1, side, at)
    h["b"] = np.where(flags & RUNS2, np.where(flags & RUNS1, 0, side), other)
    h["row"], h["len"], h["flags"] = rnd.randint(0, 1 << 32, n, dtype=np.uint64), L, flags
    return h


def window_cuts(n_pos, n_tiles, forced):
    """(n_win, [win_tile[0..n_win]]) of agx::window_cuts"""
    cuts = np.zeros(9, np.uint32)
    n = lib().agx_forms_window_cuts(n_pos, n_tiles, forced, cuts.ctypes.data)
    return int(n), [int(x) for x in cuts[:n + 1]]


def row_piece(nh, stride, win_tile, tile_first, other_t, w_lo, w_hi, block_off=None, n_rowcnt=0):
    """agx::row_piece as a dict; block_off: the rows cross as differences"""
    c = np.array([nh, stride, len(win_tile) - 1, n_rowcnt, len(other_t)], np.uint64)
    wt, tf, ot = np.zeros(9, np.uint32), np.ascontiguousarray(tile_first, np.uint32), np.ascontiguousarray(np.append(other_t, 0), np.uint64)
    wt[:len(win_tile)] = win_tile
    bo = np.ascontiguousarray(block_off if block_off is not None else [0], np.uint32)
    out = np.zeros(14, np.uint64)
    lib().agx_forms_row_piece(c.ctypes.data, wt.ctypes.data, tf.ctypes.data, int(block_off is not None), bo.ctypes.data, ot.ctypes.data, w_lo, w_hi, out.ctypes.data)
    return dict(zip(PIECE_FIELDS, (int(x) for x in out)))
