// agx_forms.h — the upload forms of a unit's read alignments as index arithmetic over plain arrays: the tile-ordered gather, the compact hit and side packers, the cuts of the
// upload windows, a window's piece of the rows, and whether the rows gain anything as differences from the reference.  No device, no pinned memory: destination memory is
// always the caller's (the engine: PBuf, agx_engine.cpp "staging"; the tests: numpy arrays and exact-size heap blocks), so what the engine stages is what the CPU tests and
// the stand-alone sanitizer programs run.  Which forms a unit takes is the engine's UploadChoice (agx_unit.h), read once per entry; the inputs are named by StagedView.
#pragma once
#include "agx_host.h"

namespace agx {

// The hit and side records of the upload in their compact wire forms (agx_core.h "compact wire forms"): 16 -> about 9.5 bytes per hit and 12 -> 2 per side cross PCIe, in
// front of everything else a unit sends, and the device makes d_whits / d_wsides of them at the head of the unit's first build (agx_k_expand_hits, agx_k_side_*).
// The hits, a block at a time as its 64 records stand in the upload's order `hits` (tile order: gather_tiled writes them in its loop and hands each block over while it
// is in the cache; file order: pack_blocks).  Thread t of T packs the blocks [first(t), first(t + 1)); its escapes and extra words collect in lists of its own and
// the headers hold places in those until finish() has put the lists behind one another.  Everything lands in ONE buffer of the size the records would have taken
// (`wire`, (nh + 1) * sizeof(agx_whit) bytes: blocks, escapes, extra words — they are used only where they are fewer bytes).
struct HitWire { bool gain; size_t bytes, n_blocks, n_esc, n_ext; const agx_whit *esc; const agx_u32 *ext; };      // bytes: blocks + escapes + extra words; esc / ext: inside `wire`, where gain
struct HitPacker {
    size_t nh; agx_u32 maxlen; unsigned T; size_t n_blocks; bool on; char *wire = nullptr; std::vector<std::vector<agx_whit>> esc; std::vector<std::vector<agx_u32>> ext;
    HitPacker(size_t n_hits, agx_u32 longest, unsigned threads, bool compact) : nh(n_hits), maxlen(longest), T(threads), n_blocks((n_hits + AGX_CH_BLOCK - 1) / AGX_CH_BLOCK), esc(threads), ext(threads) {
        on = compact && n_blocks * sizeof(agx_chit_block) < nh * sizeof(agx_whit);      // (a few dozen hits: the last block's empty slots outweigh the rest)
    }
    void into(char *buffer) { wire = buffer; for (unsigned t = 0; t < T; t++) { esc[t].reserve(nh / T / 8 + 64); ext[t].reserve(nh / T / 2 + 64); } }      // (only where `on`)
    agx_chit_block *blocks() const { return (agx_chit_block *)wire; }
    size_t first(unsigned t) const { return n_blocks * t / T; }
    void block(unsigned t, size_t b, const agx_whit *hits) {
        const size_t lo = b * AGX_CH_BLOCK; const agx_u32 n = (agx_u32)std::min<size_t>(AGX_CH_BLOCK, nh - lo);
        agx_whit e[AGX_CH_BLOCK]; agx_u32 x[AGX_CH_BLOCK], ne = 0, nx = 0;
        agx_chit_block &B = blocks()[b];
        agx_chit_pack_block(hits + lo, n, maxlen, B, e, ne, x, nx);
        B.esc = (agx_u32)esc[t].size(); B.ext = (agx_u32)ext[t].size();
        esc[t].insert(esc[t].end(), e, e + ne); ext[t].insert(ext[t].end(), x, x + nx);
    }
    void pack_blocks(const agx_whit *hits) { on_threads(T, [&](unsigned t) { for (size_t b = first(t); b < first(t + 1); b++) block(t, b, hits); }); }      // every block of an array that stands whole
    // finish() in its two halves.  The engine only ever calls finish(); tests/wire_shim.cpp calls the halves, because its callers want every number of hits packed (it sets
    // `on` itself) and the lists in arrays of their own, not behind the blocks.
    HitWire sums() {      // the threads' lists behind one another: the headers' places become places in the whole lists; the counts, and whether the blocks gain
        HitWire W{false, 0, n_blocks, 0, 0, nullptr, nullptr};
        if (!on) return W;
        size_t ne = 0, nx = 0;
        for (unsigned t = 0; t < T; t++) { for (size_t b = first(t); b < first(t + 1); b++) { blocks()[b].esc += (agx_u32)ne; blocks()[b].ext += (agx_u32)nx; } ne += esc[t].size(); nx += ext[t].size(); }
        W.n_esc = ne; W.n_ext = nx; W.bytes = n_blocks * sizeof(agx_chit_block) + ne * sizeof(agx_whit) + nx * 4;
        W.gain = W.bytes < nh * sizeof(agx_whit);
        return W;
    }
    void lists(agx_whit *e_at, agx_u32 *x_at) const {
        for (unsigned t = 0; t < T; t++) {
            if (!esc[t].empty()) memcpy(e_at, esc[t].data(), esc[t].size() * sizeof(agx_whit));
            if (!ext[t].empty()) memcpy(x_at, ext[t].data(), ext[t].size() * 4);
            e_at += esc[t].size(); x_at += ext[t].size();
        }
    }
    HitWire finish() {      // gain false: the blocks would be no fewer bytes than the records (hits all over the unit: file order) — the unit sends its records
        HitWire W = sums();
        if (!W.gain) return W;
        agx_whit *e_at = (agx_whit *)(wire + n_blocks * sizeof(agx_chit_block)); agx_u32 *x_at = (agx_u32 *)(e_at + W.n_esc);      // (a block is a multiple of 16 bytes)
        W.esc = e_at; W.ext = x_at;
        lists(e_at, x_at);
        return W;
    }
};

// The sides as their counts, the listed sides behind them in one buffer.  The run pool lies in side order (both loaders write a hit's runs where the last hit's end) or
// the unit sends the records themselves: plan_sides is that check (agx_sides_consecutive, a side at a time) with the count of the sides that need listing beside it.
struct SidePlan { bool in_order, fine; agx_u32 first; size_t listed, bytes, counts_bytes; };      // fine: in order, and fewer bytes than the records; counts_bytes: where the listed sides begin
inline SidePlan plan_sides(const agx_wside *sd, size_t n) {
    SidePlan P{true, false, agx_cside_first(sd, n), 0, 0, 0};
    unsigned long long at = P.first;
    for (size_t i = 0; i < n && P.in_order; i++) { P.in_order = agx_cside_in_order(sd[i], at); P.listed += agx_cside_pack(sd[i].nruns) == AGX_CS_ESC; }
    P.counts_bytes = (n * 2 + 7) & ~(size_t)7; P.bytes = n * 2 + P.listed * sizeof(agx_cside_esc);
    P.fine = P.in_order && P.bytes < n * sizeof(agx_wside);
    return P;
}
// counts: n entries; listed: the plan's `listed` entries
inline void fill_sides(const agx_wside *sd, size_t n, agx_u16 *c, agx_cside_esc *l) {
    for (size_t i = 0; i < n; i++) { const agx_u32 v = agx_cside_pack(sd[i].nruns); c[i] = (agx_u16)v; if (v == AGX_CS_ESC) *l++ = agx_cside_esc{(agx_u32)i, sd[i].nruns}; }
}

// What the device is sent of the read alignments, in the order of the hits' first tiles (order_hits' permutation applied on the host).
//   * the wire records: hits_t[i] = hit perm[i], its `row` field carrying the hit's NUMBER (the key the tile lists are ranked by) — the 4 bytes per hit of the permutation no
//     longer cross PCIe, the device reads the records in order instead of gathering them — and AGX_WF_DUP what the rule of AG:1650-1655 says about it (it needs the hit's FILE
//     neighbours, which are not its neighbours here);
//   * the read rows: row i of codes_t = the left-mate row of the i-th hit (a pair with a second hit sends its row twice: 5 % of the rows), so the rows that a WINDOW of tiles
//     reads are one contiguous piece of the upload, in front of which lie the rows of every earlier tile: the unit's first build sweeps window w when its piece has landed,
//     beside the upload of the pieces behind it — chr1 of configs[4]: 22 ms of node sweep that used to wait for the last read row;
//   * the list of the bases that are not A, C, G, T, re-indexed to those rows: what is returned, ascending.
// The k-mer string references of the nodes then name places in the tile order: slot_row maps them back for the walk (UnitView::slot_row).
// V: the staged arrays in file order, `codes` their packed rows (V.stride / 4 bytes each).  hits_t: V.nh + 1 records; codes_t: V.nh * (V.stride / 4) + 16 bytes; slot_row: V.nh
// entries.  A thread takes whole blocks of 64 hits and hands each finished block to the packer (made for the same T) while it is in the cache.
inline std::vector<unsigned long long> gather_tiled(const StagedView &V, const agx_u8 *codes, const agx_u32 *perm, unsigned T, HitPacker &packer, agx_whit *hits_t, agx_u8 *codes_t, agx_u32 *slot_row) {
    const size_t nh = V.nh, s4 = V.stride / 4;
    const agx_whit *wh = V.hits; const agx_wside *sd = V.sides; const agx_wrun *wr = V.runs;
    // rows that carry a listed base (few): one bit per row
    const size_t n_rows = (size_t)V.n_rows; std::vector<agx_u8> has_other((n_rows + 7) / 8, 0);
    for (size_t j = 0; j < V.n_other; j++) { const size_t r = (size_t)(V.other[j] / V.stride); if (r < n_rows) has_other[r >> 3] |= (agx_u8)(1u << (r & 7)); }
    auto idx0 = [&](const agx_whit &w) -> agx_u32 {      // positionSets[hit][0] of mate1 (agx_idx0_pos on the wire forms)
        if (!(w.flags & AGX_WF_RUNS1)) return w.a;
        const agx_wside &g = sd[w.a]; const agx_wrun &r = wr[g.runs1];
        return r.q == 0 ? r.t : AGX_NONE;
    };
    std::vector<std::vector<unsigned long long>> others(T);
    const size_t n_blocks = (nh + AGX_CH_BLOCK - 1) / AGX_CH_BLOCK;      // (a thread takes whole blocks of 64 hits)
    on_threads(T, [&](unsigned t) {
        // (two dependent random reads per hit — its record, then its row: asked for a few hits ahead, or every hit costs two cache misses in a row: 0.16 s of cfg3's load)
        const size_t AHEAD = 48, NEAR = 24;
        for (size_t i = (n_blocks * t / T) * AGX_CH_BLOCK, hi = std::min<size_t>(nh, (n_blocks * (t + 1) / T) * AGX_CH_BLOCK); i < hi; i++) {
            if (i + AHEAD < hi) __builtin_prefetch(wh + perm[i + AHEAD]);
            if (i + NEAR < hi) { const char *c = (const char *)(codes + (size_t)wh[perm[i + NEAR]].row * s4); __builtin_prefetch(c); if (s4 > 40) __builtin_prefetch(c + 64); }
            const agx_u32 h = perm[i]; agx_whit w = wh[h];
            const agx_u32 row = w.row;
            slot_row[i] = row;
            memcpy(codes_t + i * s4, codes + (size_t)row * s4, s4);
            bool dup = false;
            if (w.back) { const agx_u32 me = idx0(w); for (agx_u32 e = 1; e <= w.back && !dup; e++) dup = agx_absdiff(me, idx0(wh[h - e])) < (int)w.len; }      // agx_hit_dup_by
            w.row = h; if (dup) w.flags |= (agx_u8)AGX_WF_DUP;
            hits_t[i] = w;
            if (packer.on && ((i & (AGX_CH_BLOCK - 1)) == AGX_CH_BLOCK - 1 || i + 1 == nh)) packer.block(t, i / AGX_CH_BLOCK, hits_t);
            if (has_other[row >> 3] & (1u << (row & 7))) {
                const unsigned long long lo = (unsigned long long)row * V.stride, *b = V.other, *e = b + V.n_other;
                for (const unsigned long long *at = std::lower_bound(b, e, lo); at != e && *at < lo + V.stride; ++at) others[t].push_back((unsigned long long)i * V.stride + (*at - lo));
            }
        }
    });
    size_t no = 0; for (auto &v : others) no += v.size();
    std::vector<unsigned long long> list; list.reserve(no);
    for (auto &v : others) list.insert(list.end(), v.begin(), v.end());
    return list;
}

// Windows of the first build's sweep: about 8 M positions each, eight at most (`forced` != 0: that many, tests), cut at tiles: window w = tiles [win_tile[w], win_tile[w + 1]).
// Returns how many there are.
inline agx_u32 window_cuts(size_t n_pos, size_t n_tiles, unsigned forced, agx_u32 win_tile[9]) {
    size_t W = forced ? (size_t)forced : n_pos / 8000000u;
    W = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(W, 8), n_tiles));
    for (size_t w = 0; w <= W; w++) win_tile[w] = (agx_u32)(n_tiles * w / W);
    return (agx_u32)W;
}

// The read rows of windows [w_lo, w_hi) of a tile-ordered unit ((0, n_win): all of them), named ONCE for both sides of the upload: the upload copies what a piece names and
// the unit's first build expands the same piece into the vote codes.  File-order units have none.
struct RowPiece { size_t r_lo, r_hi,      // the rows: those of the hits whose first tile lies in the windows (a tile's list also names hits that begin in earlier tiles: earlier pieces)
    code_lo, code_hi,      // 2-bit rows: their bytes in codes_t
    cnt_lo, cnt_hi, blk_lo, blk_hi, unit_lo, unit_hi,      // rows as differences: count bytes, whole 64-row blocks (block_off, block_first), their 16-bit units
    v_lo, v_hi, o_lo, o_hi; };      // the bases of the vote codes they are expanded to; the listed bases among them: entries of the tile-ordered list
struct RowWindows {      // what a piece is cut by
    size_t nh; agx_u32 stride, n_win; const agx_u32 *win_tile, *tile_first;      // tile_first: order_hits'
    bool rows_diffed; size_t n_rowcnt; const agx_u32 *block_off;      // (RowDiffs: cnt.size(), block_off)
    const unsigned long long *other_t; size_t n_other_t;      // gather_tiled's list
};
inline RowPiece row_piece(const RowWindows &u, agx_u32 w_lo, agx_u32 w_hi) {
    // a window's first row: the place in the tile order of the first hit of its first tile, rounded up to 16 rows — a piece then begins on a 16-byte boundary of the packed
    // classes and on a multiple of 16 bases (agx_k_expand_codes takes 16 bases per thread) —, to 64 where the rows cross as differences (whole blocks of the stream); the few
    // rows of the next window's hits that ride in this piece only arrive early
    const size_t a = u.rows_diffed ? 63 : 15, s4 = u.stride / 4, nh = u.nh;
    auto first_row = [&](agx_u32 w) { return w == 0 ? 0 : w >= u.n_win ? nh : std::min(nh, ((size_t)u.tile_first[u.win_tile[w]] + a) & ~a); };
    const unsigned long long *ob = u.other_t, *oe = ob + u.n_other_t;
    auto listed_at = [&](size_t row) { return (size_t)(std::lower_bound(ob, oe, (unsigned long long)row * u.stride) - ob); };
    RowPiece p{}; p.r_lo = first_row(w_lo); p.r_hi = first_row(w_hi); p.o_lo = listed_at(p.r_lo); p.o_hi = listed_at(p.r_hi);
    if (u.rows_diffed) {
        p.blk_lo = p.r_lo / 64; p.blk_hi = (p.r_hi + 63) / 64; p.cnt_lo = p.r_lo; p.cnt_hi = std::min<size_t>(u.n_rowcnt, p.blk_hi * 64);
        p.unit_lo = u.block_off[p.blk_lo]; p.unit_hi = u.block_off[p.blk_hi];
    } else { p.code_lo = p.r_lo * s4; p.code_hi = p.r_hi * s4; }
    // the piece that holds the LAST row — not always the last window's: a unit with few hits has windows without rows — is padded to whole 16-base groups like the whole array
    // (r06's fuzz found the unpadded form: the last row's last bases stayed unexpanded where an earlier window already reached the last row)
    p.v_lo = p.r_lo * s4 * 4; p.v_hi = p.r_hi == nh ? (nh * s4 * 4 + 15) / 16 * 16 : p.r_hi * s4 * 4;
    return p;
}

// The read rows as differences from the reference (build_row_diffs): the bytes the form sends, and whether that is fewer than the 2-bit rows' `rows_bytes` (reads that do
// not resemble the reference gain nothing: the unit sends its 2-bit rows)
inline size_t row_diffs_bytes(const RowDiffs &D) { return D.n_units * 2 + D.cnt.size() + (D.block_off.size() + D.block_first.size() + D.anchor_bits.size()) * 4; }
inline bool row_diffs_gain(const RowDiffs &D, size_t rows_bytes) { return row_diffs_bytes(D) < rows_bytes; }

}  // namespace agx
