// wire_shim.cpp — TEST-ONLY: the compact wire forms of the hit and side records (csrc/agx_core.h "compact wire forms") over arrays handed in from numpy.  The packing is
// the engine's: agx_chit_pack_block per block of 64 with the running sums in the headers (HitPacker, agx_engine.cpp), agx_cside_pack per side behind the check that the run
// pool lies in side order.  The way back is the device's, with its wavefront instructions as plain loops: per slot agx_chit_escaped / agx_chit_decode and a count of the
// escapes and extra words in front of the lane (agx_k_expand_hits' ballots); per side the counts, the listed sides over them, an exclusive scan, agx_cside_rebuild
// (agx_k_side_counts, agx_k_side_listed, agx_k_side_firsts).  tests/test_wire_codec.py compiles this into a shared library with g++.  With -DAGX_WIRE_SHIM_MAIN it is
// a program of its own (for a sanitizer build): random records of every kind through both ways.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_core.h"

// blocks: (n + 63) / 64 of them; esc: room for n records; ext: room for n words; counts[0..1] = escapes, extra words
extern "C" void agx_wire_pack_hits(const agx_whit *hits, uint32_t n, uint32_t maxlen, agx_chit_block *blocks, agx_whit *esc, uint32_t *ext, uint32_t *counts) {
    uint32_t ne = 0, nx = 0;
    for (uint32_t b = 0; b * AGX_CH_BLOCK < n; b++) {
        const uint32_t m = n - b * AGX_CH_BLOCK < AGX_CH_BLOCK ? n - b * AGX_CH_BLOCK : AGX_CH_BLOCK;
        uint32_t e = 0, x = 0;
        agx_chit_pack_block(hits + (size_t)b * AGX_CH_BLOCK, m, maxlen, blocks[b], esc + ne, e, ext + nx, x);
        blocks[b].esc = ne; blocks[b].ext = nx; ne += e; nx += x;
    }
    counts[0] = ne; counts[1] = nx;
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
    *n_listed = 0;
    if (!agx_sides_consecutive(sides, n, *first)) return 0;
    for (uint32_t i = 0; i < n; i++) { const uint32_t c = agx_cside_pack(sides[i].nruns); counts[i] = (uint16_t)c; if (c == AGX_CS_ESC) listed[(*n_listed)++] = agx_cside_esc{i, sides[i].nruns}; }
    return 1;
}
extern "C" void agx_wire_unpack_sides(const uint16_t *counts, uint32_t n, const agx_cside_esc *listed, uint32_t n_listed, uint32_t first, agx_wside *out) {
    std::vector<uint32_t> total(n + 1, 0u), before(n + 1, 0u);
    for (uint32_t i = 0; i < n; i++) { const uint32_t nr = agx_cside_nruns(counts[i]); out[i].nruns = nr; total[i] = agx_cside_total(nr); }
    for (uint32_t j = 0; j < n_listed; j++) { out[listed[j].side].nruns = listed[j].nruns; total[listed[j].side] = agx_cside_total(listed[j].nruns); }
    for (uint32_t i = 0; i < n; i++) before[i + 1] = before[i] + total[i];
    for (uint32_t i = 0; i < n; i++) out[i] = agx_cside_rebuild(first, before[i], out[i].nruns);
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
            agx_wire_pack_hits(h.data(), n, maxlen, B.data(), esc.data(), ext.data(), counts);
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
