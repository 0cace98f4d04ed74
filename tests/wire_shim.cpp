// wire_shim.cpp — TEST-ONLY: the upload forms of a unit's read alignments (csrc/agx_forms.h) over arrays handed in from numpy.  The packing is the product's own: HitPacker
// (agx_chit_pack_block per block of 64 with the running sums in the headers) and plan_sides / fill_sides (agx_cside_pack per side behind the check that the run pool lies in
// side order), called here as the engine's staging calls them; so are the tile-ordered gather, the window cuts and a window's piece of the rows (tests/test_stage_forms.py).
// The way back is the device's, with its wavefront instructions as plain loops: per slot agx_chit_escaped / agx_chit_decode and a count of the
// escapes and extra words in front of the lane (agx_k_expand_hits' ballots); per side the counts, the listed sides over them, an exclusive scan, agx_cside_rebuild
// (agx_k_side_counts, agx_k_side_listed, agx_k_side_firsts).  tests/test_wire_codec.py compiles this into a shared library with g++.  With -DAGX_WIRE_SHIM_MAIN it is
// a program of its own (for a sanitizer build): random records of every kind through both ways.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_forms.h"

// blocks: (n + 63) / 64 of them; esc: room for n records; ext: room for n words; counts[0..1] = escapes, extra words.  The product's packer on `threads` threads, made to
// pack whatever the number of hits (the engine leaves a few dozen as they are), its lists laid where the caller wants them.
extern "C" void agx_wire_pack_hits(const agx_whit *hits, uint32_t n, uint32_t maxlen, uint32_t threads, agx_chit_block *blocks, agx_whit *esc, uint32_t *ext, uint32_t *counts) {
    agx::HitPacker P(n, maxlen, threads ? threads : 1u, true);
    P.on = true; P.into((char *)blocks);
    P.pack_blocks(hits);
    const agx::HitWire W = P.sums();
    P.lists(esc, ext);
    counts[0] = (uint32_t)W.n_esc; counts[1] = (uint32_t)W.n_ext;
}
// the same as the engine runs it: wire: (n + 1) * sizeof(agx_whit) bytes; out[0..6] = the packer is on, the blocks gained, blocks, escapes, extra words, where in `wire` the
// escapes and the extra words begin (0 without gain)
extern "C" void agx_forms_pack_wire(const agx_whit *hits, uint32_t n, uint32_t maxlen, uint32_t threads, char *wire, uint64_t *out) {
    agx::HitPacker P(n, maxlen, threads ? threads : 1u, true);
    if (P.on) { P.into(wire); P.pack_blocks(hits); }
    const agx::HitWire W = P.finish();
    out[0] = P.on; out[1] = W.gain; out[2] = W.n_blocks; out[3] = W.n_esc; out[4] = W.n_ext;
    out[5] = W.gain ? (uint64_t)((const char *)W.esc - wire) : 0; out[6] = W.gain ? (uint64_t)((const char *)W.ext - wire) : 0;
}
// a lane per slot: what lane `lane` of block b stores
static agx_whit lane_of_block(const agx_chit_block &B, uint32_t lane, uint32_t valid, uint32_t maxlen, const agx_whit *esc, const uint32_t *ext) {
    uint32_t e = 0, x = 0;      // the ballots' bits in front of the lane
    for (uint32_t l = 0; l < lane && l < valid; l++) { if (agx_chit_escaped(B.word[l])) e++; else if (agx_chit_has_side(B.word[l])) x++; }
    const uint32_t word = B.word[lane];
    if (agx_chit_escaped(word)) return esc[B.esc + e];
    return agx_chit_decode(B.num[lane], word, B.base, maxlen, agx_chit_has_side(word) ? ext[B.ext + x] : 0u);
}
extern "C" void agx_wire_unpack_hits(const agx_chit_block *blocks, uint32_t n, uint32_t maxlen, const agx_whit *esc, const uint32_t *ext, agx_whit *out) {
    for (uint32_t i = 0; i < n; i++) { const uint32_t b = i / AGX_CH_BLOCK, valid = n - b * AGX_CH_BLOCK < AGX_CH_BLOCK ? n - b * AGX_CH_BLOCK : AGX_CH_BLOCK; out[i] = lane_of_block(blocks[b], i % AGX_CH_BLOCK, valid, maxlen, esc, ext); }
}
// the host's slot-by-slot way back (agx_chit_unpack_block), which must agree with the lanes'
extern "C" void agx_wire_unpack_hits_serial(const agx_chit_block *blocks, uint32_t n, uint32_t maxlen, const agx_whit *esc, const uint32_t *ext, agx_whit *out) {
    for (uint32_t b = 0; b * AGX_CH_BLOCK < n; b++) agx_chit_unpack_block(blocks[b], n - b * AGX_CH_BLOCK < AGX_CH_BLOCK ? n - b * AGX_CH_BLOCK : AGX_CH_BLOCK, maxlen, esc, ext, out + (size_t)b * AGX_CH_BLOCK);
}
// 1: packed (counts[n], listed: room for n entries, *n_listed, *first); 0: the run pool is not in side order — the unit sends its records
extern "C" int agx_wire_pack_sides(const agx_wside *sides, uint32_t n, uint16_t *counts, agx_cside_esc *listed, uint32_t *n_listed, uint32_t *first) {
    const agx::SidePlan P = agx::plan_sides(sides, n);
    *n_listed = 0; *first = P.first;
    if (!P.in_order) return 0;
    agx::fill_sides(sides, n, counts, listed); *n_listed = (uint32_t)P.listed;
    return 1;
}
extern "C" void agx_wire_unpack_sides(const uint16_t *counts, uint32_t n, const agx_cside_esc *listed, uint32_t n_listed, uint32_t first, agx_wside *out) {
    std::vector<uint32_t> total(n + 1, 0u), before(n + 1, 0u);
    for (uint32_t i = 0; i < n; i++) { const uint32_t nr = agx_cside_nruns(counts[i]); out[i].nruns = nr; total[i] = agx_cside_total(nr); }
    for (uint32_t j = 0; j < n_listed; j++) { out[listed[j].side].nruns = listed[j].nruns; total[listed[j].side] = agx_cside_total(listed[j].nruns); }
    for (uint32_t i = 0; i < n; i++) before[i + 1] = before[i] + total[i];
    for (uint32_t i = 0; i < n; i++) out[i] = agx_cside_rebuild(first, before[i], out[i].nruns);
}

// The tile-ordered gather with the hits packed inside it (gather_tiled), as stage_tiled runs it.  c[0..7] = hits, sides, runs, listed bases, rows, stride, the longest read,
// room in other_t; wire, hits_t: (nh + 1) records' bytes; codes_t: nh * (stride / 4) + 16 bytes; slot_row: nh entries; out: as agx_forms_pack_wire's.  Returns the entries
// of the re-indexed list (the first c[7] of them are written).
extern "C" uint64_t agx_forms_gather(const uint64_t *c, const agx_whit *hits, const agx_wside *sides, const agx_wrun *runs, const unsigned long long *other, const uint8_t *codes, const uint32_t *perm,
                                     uint32_t threads, int compact, char *wire, agx_whit *hits_t, uint8_t *codes_t, uint32_t *slot_row, unsigned long long *other_t, uint64_t *out) {
    agx::StagedView V; V.hits = hits; V.nh = (size_t)c[0]; V.sides = sides; V.n_sides = (size_t)c[1]; V.runs = runs; V.n_runs = (size_t)c[2]; V.other = other; V.n_other = (size_t)c[3];
    V.n_rows = c[4]; V.stride = (uint32_t)c[5]; V.maxlen = (uint32_t)c[6];
    const unsigned T = threads ? threads : 1u;
    agx::HitPacker P(V.nh, V.maxlen, T, compact != 0);
    if (P.on) P.into(wire);
    const std::vector<unsigned long long> list = agx::gather_tiled(V, codes, perm, T, P, hits_t, codes_t, slot_row);
    const agx::HitWire W = P.finish();
    out[0] = P.on; out[1] = W.gain; out[2] = W.n_blocks; out[3] = W.n_esc; out[4] = W.n_ext;
    out[5] = W.gain ? (uint64_t)((const char *)W.esc - wire) : 0; out[6] = W.gain ? (uint64_t)((const char *)W.ext - wire) : 0;
    for (size_t i = 0; i < list.size() && i < c[7]; i++) other_t[i] = list[i];
    return list.size();
}
extern "C" uint32_t agx_forms_window_cuts(uint64_t n_pos, uint64_t n_tiles, uint32_t forced, uint32_t *win_tile /* 9 */) { return agx::window_cuts((size_t)n_pos, (size_t)n_tiles, forced, win_tile); }
// c[0..4] = hits, stride, windows, count bytes of the rows' differences, listed bases; out[0..13]: the piece's fields in their order
extern "C" void agx_forms_row_piece(const uint64_t *c, const uint32_t *win_tile, const uint32_t *tile_first, int rows_diffed, const uint32_t *block_off, const unsigned long long *other_t,
                                    uint32_t w_lo, uint32_t w_hi, uint64_t *out) {
    const agx::RowPiece p = agx::row_piece(agx::RowWindows{(size_t)c[0], (uint32_t)c[1], (uint32_t)c[2], win_tile, tile_first, rows_diffed != 0, (size_t)c[3], block_off, other_t, (size_t)c[4]}, w_lo, w_hi);
    const size_t f[14] = {p.r_lo, p.r_hi, p.code_lo, p.code_hi, p.cnt_lo, p.cnt_hi, p.blk_lo, p.blk_hi, p.unit_lo, p.unit_hi, p.v_lo, p.v_hi, p.o_lo, p.o_hi};
    for (int i = 0; i < 14; i++) out[i] = f[i];
}

#ifdef AGX_WIRE_SHIM_MAIN
int main() {
    uint32_t x = 2463534242u; auto rnd = [&] { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    int bad = 0;
    for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 128u, 129u, 5000u}) {
        for (int kind = 0; kind < 4; kind++) {      // 0: any record; 1: records the loaders make, close together; 2: the same with escapes of every cause among them; 3: all escaped
            const uint32_t maxlen = 150;
            std::vector<agx_whit> h(n), out(n), out2(n), esc(n + 1); std::vector<uint32_t> ext(n + 1); std::vector<agx_chit_block> B(n / AGX_CH_BLOCK + 1);
            for (uint32_t i = 0; i < n; i++) {
                agx_whit w;
                if (kind == 0) { w.a = rnd(); w.b = rnd(); w.row = rnd(); w.len = (uint16_t)rnd(); w.flags = (uint8_t)rnd(); w.back = (uint8_t)rnd(); }
                else {
                    const uint32_t at = 100000u + i * 7u + rnd() % 64u;
                    w.flags = (uint8_t)(rnd() & 63u); w.row = rnd(); w.len = (uint16_t)maxlen; w.back = 0;
                    w.a = (w.flags & AGX_WF_RUNS1) ? rnd() : at; w.b = (w.flags & AGX_WF_RUNS2) ? ((w.flags & AGX_WF_RUNS1) ? 0u : rnd()) : at + 300u + rnd() % 100u;
                    if (kind == 2 && rnd() % 5u == 0) { switch (rnd() % 4u) { case 0: w.len = 77; break; case 1: w.back = 3; break; case 2: w.flags |= 128u; break; default: w.a += 1u << 25; } }
                    if (kind == 3) w.back = 1;
                }
                h[i] = w;
            }
            uint32_t counts[2];
            agx_wire_pack_hits(h.data(), n, maxlen, 1u + (uint32_t)kind, B.data(), esc.data(), ext.data(), counts);      // (on 1 to 4 threads)
            if (kind == 3 && counts[0] != n) bad++;
            agx_wire_unpack_hits(B.data(), n, maxlen, esc.data(), ext.data(), out.data());
            agx_wire_unpack_hits_serial(B.data(), n, maxlen, esc.data(), ext.data(), out2.data());
            if (n && (memcmp(h.data(), out.data(), n * sizeof(agx_whit)) != 0 || memcmp(h.data(), out2.data(), n * sizeof(agx_whit)) != 0)) bad++;
        }
        for (int kind = 0; kind < 3; kind++) {      // 0: small counts; 1: counts beyond a byte among them; 2: a pool out of side order
            std::vector<agx_wside> s(n), out(n); std::vector<uint16_t> c(n + 1); std::vector<agx_cside_esc> listed(n + 1);
            uint32_t at = 17;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t n1 = kind == 1 && rnd() % 7u == 0 ? 250u + rnd() % 20u : rnd() % 5u, n2 = kind == 1 && rnd() % 9u == 0 ? 65535u : rnd() % 4u;
                if (!(n1 | n2)) { s[i] = agx_wside{at, 0u, 1u}; at += 1; continue; }      // (a side record has a mate with runs; one without holds a zero)
                s[i] = agx_wside{n1 ? at : 0u, n2 ? at + n1 : 0u, n1 | n2 << 16}; at += n1 + n2;
            }
            if (kind == 2 && n > 1) s[n / 2].runs1 += 1;
            uint32_t nl = 0, first = 0;
            const int ok = agx_wire_pack_sides(s.data(), n, c.data(), listed.data(), &nl, &first);
            if (ok != (kind == 2 && n > 1 ? 0 : 1)) { bad++; continue; }
            if (!ok) continue;
            agx_wire_unpack_sides(c.data(), n, listed.data(), nl, first, out.data());
            if (n && memcmp(s.data(), out.data(), n * sizeof(agx_wside)) != 0) bad++;
        }
    }
    printf("wire shim: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
