"""A plain model of the binning in front of the node sweep: which hits reach which tile, in which order, and through which arm of the device's list kernels.

Input: the serial executor's derived hit records in FILE order (only their fields x_lo, x_hi and flags), the unit's positions, the longest read's length and k.
Nothing of the project is imported: this is numpy over three columns.  What it states (agx_k_hit_prep, the scan, agx_k_tile_fill / agx_tile_fill_general, agx_k_bin_fill and
agx_k_tile_sort in agx_kernels.hip must all agree with it):

  * a hit is kept unless its SKIP flag is set; a kept hit reaches the tiles x_lo // 64 .. x_hi // 64;
  * tile_cnt[t] = kept hits that reach t, tile_off = its exclusive prefix sum, and tile t's list = those hits in ascending file number;
  * the device's order of the hits = a stable sort of ALL hits by first tile; tile_first[t] = hits in front of tile t's own.  A kept hit's first tile is x_lo // 64.  A
    skipped hit has no arrivals, so the records say nothing about where the staging puts it: the caller names the first aligned position of its left mate (skip_x);
  * lookback = 1 + ceil((L - k) / 64) tiles, between 2 and 16: a read's arrivals span L - k + 1 positions, so a hit without a long deletion ends less than `lookback`
    tiles behind its first one.  The others (t1 - t0 >= lookback) are the long hits;
  * ckey[i] = last tile of the hit at place i of the order, NONE for skipped and long hits;
  * dense_lists = 0 without long hits, 1 with up to LONG_MAX of them, 2 beyond;
  * the arm a tile's list is made by: see arms().
"""
import numpy as np

TILE = 64
NONE = 0xFFFFFFFF
SKIP = 2                 # AGX_HF_SKIP
LONG_MAX = 1024          # long hits the list of long hits takes
SORT_LDS = 512           # list entries a rank sort holds in LDS
FAST_WINDOW = 64         # hits of a window the fast form of agx_k_tile_fill takes (a lane each)
LOOKBACK_MAX = 16


def lookback(L, k):
    return min(max(1 + (max(L - k, 0) + TILE - 1) // TILE, 2), LOOKBACK_MAX)


def build(dhit, n_pos, L, k, skip_x=None):
    """dhit: structured array with x_lo, x_hi, flags (file order).  skip_x: {file number: first aligned position of the left mate} for every skipped hit."""
    nh = len(dhit)
    n_tiles = (n_pos + TILE - 1) // TILE
    kept = (dhit["flags"].astype(np.int64) & SKIP) == 0
    t0 = np.where(kept, dhit["x_lo"].astype(np.int64) // TILE, 0)
    t1 = np.where(kept, dhit["x_hi"].astype(np.int64) // TILE, 0)
    assert np.all(t0[kept] <= t1[kept]) and (not kept.any() or dhit["x_hi"][kept].max() < n_pos)
    lb = lookback(L, k)
    first_tile = t0.copy()
    for h in np.nonzero(~kept)[0]:
        assert skip_x is not None and int(h) in skip_x, "the model needs the left mate's first position of skipped hit %d" % h
        first_tile[h] = min(skip_x[int(h)] // TILE, n_tiles - 1)
    # lists: (tile, hit) pairs in (tile, hit) order
    hk = np.nonzero(kept)[0]
    span = (t1 - t0 + 1)[hk]
    e_hit = np.repeat(hk, span)
    e_tile = np.repeat(t0[hk], span) + (np.arange(span.sum()) - np.repeat(np.cumsum(span) - span, span))
    o = np.lexsort((e_hit, e_tile))
    e_hit, e_tile = e_hit[o], e_tile[o]
    tile_cnt = np.bincount(e_tile, minlength=n_tiles + 1).astype(np.int64)          # (entry n_tiles: 0)
    tile_off = np.concatenate(([0], np.cumsum(tile_cnt[:n_tiles])))
    order = np.argsort(first_tile, kind="stable")
    tile_first = np.searchsorted(first_tile[order], np.arange(n_tiles + 1), side="left")
    lng = kept & (t1 - t0 >= lb)
    ckey = np.where(kept & ~lng, t1, NONE)[order]
    n_long = int(lng.sum())
    return {"n_hits": nh, "n_tiles": n_tiles, "lookback": lb, "kept": kept, "t0": t0, "t1": t1, "first_tile": first_tile, "tile_cnt": tile_cnt, "tile_off": tile_off,
            "entry_hit": e_hit, "entry_tile": e_tile, "order": order, "tile_first": tile_first, "ckey": ckey, "long": lng, "long_count": n_long,
            "long_hits": set(np.nonzero(lng)[0].tolist()), "dense_lists": 0 if n_long == 0 else 1 if n_long <= LONG_MAX else 2}


def tile_list(m, t):
    return m["entry_hit"][m["tile_off"][t]:m["tile_off"][t + 1]]


def arms(m):
    """Per tile, the arm of the list kernels that makes its list: "empty", "fast" (agx_k_tile_fill's two-tile form: no long hit in the unit and a window of at most 64 hits),
    "general_lds" / "general_global" (agx_tile_fill_general with a list of up to / beyond 512 entries), "dense_lds" / "dense_global" (agx_k_tile_sort, units with more than
    1 024 long hits).  Also the window widths: width[t] = tile_first[t + 1] - tile_first[max(t - lookback + 1, 0)]."""
    nt, lb = m["n_tiles"], m["lookback"]
    t = np.arange(nt)
    width = m["tile_first"][t + 1] - m["tile_first"][np.maximum(t - lb + 1, 0)]
    n = m["tile_cnt"][:nt]
    arm = np.empty(nt, dtype=object)
    for i in range(nt):
        if n[i] == 0:
            arm[i] = "empty"
        elif m["dense_lists"] == 2:
            arm[i] = "dense_lds" if n[i] <= SORT_LDS else "dense_global"
        elif m["long_count"] == 0 and width[i] <= FAST_WINDOW:
            arm[i] = "fast"
        else:
            arm[i] = "general_lds" if n[i] <= SORT_LDS else "general_global"
    return arm, width
