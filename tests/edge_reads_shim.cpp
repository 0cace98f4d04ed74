// edge_reads_shim.cpp — TEST-ONLY: agx_reads_lane (csrc/agx_core.h) run serially over every (tile list entry, lane) of plain arrays, the way agx_k_edge_reads runs it on
// the device, and a serial replay of what surrounds it in agx_unit_edge_reads (csrc/agx_export.cpp): per chunk of the window's tiles a COUNT pass (selected contributions
// per position of the chunk), the exclusive scan of the counts and an EMIT pass that writes every record at its position's offset plus the lane's running count, each
// store checked against the position's count and the chunk's total; a chunk whose records do not fit `room` is counted again over half its tiles, a single tile that does
// not fit is refused (-3).  The counters e_cnt / ovf_cnt are the counting pass's (tests/edge_support_shim.cpp fills them from the same tables).
// tests/test_edge_reads_cases.py compiles both shims into one shared library and compares the records, grouped per edge, with tests/edge_reads_model.py.
//   dhit is in an order of the test's choosing: tile_hit[i] is the PLACE of entry i's hit and perm[place] its file number, as on the device.
//   out[0] records, out[1] chunks, out[2] events of the window, out[3] bad (a contribution without an edge or with a counter of 0, an index outside the tables, a list
//   entry without a hit), out[4] disagreements between the emit pass and its count.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_core.h"

extern "C" int agx_edge_reads_shim(const uint32_t *cm_start, const agx_cmkey *cm, const agx_dhit *dhit, uint32_t n_hits, const agx_run *runs,
                                   const uint32_t *tile_off, const uint32_t *tile_hit, const uint32_t *perm, uint32_t n_pos, uint32_t k, int iv,
                                   const uint32_t *node_start, const uint16_t *node_cnt, const uint32_t *nk /* [5][pool_cap]: cid, coff, cid0, coff0, off0 */, uint32_t pool_cap,
                                   const uint32_t *n_next, const uint8_t *n_flags, const agx_edge_ovf *ovf, uint32_t n_ovf, int single_ok,
                                   const uint32_t *e_cnt, const uint32_t *ovf_cnt, uint32_t pos_lo, uint32_t pos_hi, uint32_t max_support,
                                   uint32_t chunk_tiles, uint64_t room, uint32_t *recs /* [4 * cap] */, uint64_t cap, uint64_t *out) {
    agx_sweep_args A; memset(&A, 0, sizeof A);
    A.cm_start = cm_start; A.cm = cm; A.dhit = dhit; A.runs = runs; A.tile_off = tile_off; A.n_pos = n_pos; A.n_tiles = (n_pos + AGX_TILE - 1) / AGX_TILE; A.k = k; A.iv = iv;
    A.node_start = const_cast<uint32_t *>(node_start); A.node_cnt = const_cast<uint16_t *>(node_cnt); A.pool_cap = pool_cap;
    A.nk_cid = const_cast<uint32_t *>(nk); A.nk_coff = const_cast<uint32_t *>(nk + pool_cap); A.nk_cid0 = const_cast<uint32_t *>(nk + 2 * (size_t)pool_cap);
    A.nk_coff0 = const_cast<uint32_t *>(nk + 3 * (size_t)pool_cap); A.nk_off0 = const_cast<uint32_t *>(nk + 4 * (size_t)pool_cap);
    A.n_next = const_cast<uint32_t *>(n_next); A.n_flags = const_cast<uint8_t *>(n_flags);
    const agx_reads_tab T{n_next, n_flags, ovf, n_ovf, e_cnt, ovf_cnt, pos_lo, pos_hi, max_support};
    uint64_t n_recs = 0, chunks = 0, events = 0, bad = 0, disagree = 0;
    memset(out, 0, 5 * sizeof *out);
    if (pos_lo > pos_hi || pos_hi > n_pos) return -6;
    const uint32_t t_lo = pos_lo / AGX_TILE, t_hi = pos_lo < pos_hi ? (pos_hi + AGX_TILE - 1) / AGX_TILE : t_lo;
    uint32_t chunk = chunk_tiles ? chunk_tiles : (t_hi > t_lo ? t_hi - t_lo : 1u);
    // one pass over the chunk's tiles: put(p, sp, dp, vars, file number) per selected contribution of chunk position p, in the device's order
    auto pass = [&](uint32_t t0, uint32_t nt, bool count_events, auto put) {
        for (uint32_t ct = 0; ct < nt; ct++) {
            const uint32_t tile = t0 + ct;
            for (uint32_t lane = 0; lane < AGX_TILE; lane++)      // (a lane walks the whole list: the order of a position's records)
                for (uint32_t i = tile_off[tile]; i < tile_off[tile + 1]; i++) {
                    const uint32_t place = tile_hit[i];
                    if (place >= n_hits) { bad += lane == 0 && count_events; continue; }
                    bool b = false;
                    const uint32_t ev = agx_reads_lane(A, T, tile * AGX_TILE + lane, dhit[place], single_ok != 0, &b,
                                                       [&](agx_u32 sp, agx_u32 dp, agx_u32 vars) { put(ct * AGX_TILE + lane, sp, dp, vars, perm[place]); });
                    if (count_events) { events += ev; bad += b ? 1u : 0u; }
                }
        }
    };
    for (uint32_t t = t_lo; t < t_hi;) {
        uint32_t nt = chunk < t_hi - t ? chunk : t_hi - t;
        std::vector<uint32_t> cnt, off;
        uint64_t total = 0;
        for (;;) {
            cnt.assign((size_t)nt * AGX_TILE + 1, 0);
            const uint64_t ev0 = events, bad0 = bad;
            pass(t, nt, true, [&](uint32_t p, agx_u32, agx_u32, agx_u32, agx_u32) { cnt[p]++; });
            off.assign(cnt.size(), 0);
            total = 0;
            for (size_t p = 0; p < cnt.size(); p++) { off[p] = (uint32_t)total; total += cnt[p]; }
            if (total <= room) break;
            if (nt == 1) return -3;
            events = ev0; bad = bad0;      // (the chunk is counted again)
            nt = (nt + 1) / 2; chunk = nt;
        }
        chunks++;
        std::vector<uint32_t> run((size_t)nt * AGX_TILE, 0);
        pass(t, nt, false, [&](uint32_t p, agx_u32 sp, agx_u32 dp, agx_u32 vars, agx_u32 file_no) {
            const uint64_t at = (uint64_t)off[p] + run[p];
            if (run[p] < off[p + 1] - off[p] && at < total && n_recs + at < cap) { uint32_t *r = recs + 4 * (n_recs + at); r[0] = sp; r[1] = dp; r[2] = vars; r[3] = file_no; }
            else disagree++;
            run[p]++;
        });
        for (size_t p = 0; p < run.size(); p++) disagree += run[p] != off[p + 1] - off[p];
        n_recs += total;
        t += nt;
    }
    out[0] = n_recs; out[1] = chunks; out[2] = events; out[3] = bad; out[4] = disagree;
    return 0;
}
