// edge_support_shim.cpp — TEST-ONLY: agx_support_lane (csrc/agx_core.h) run serially over every (tile list entry, lane) of plain arrays, the way agx_k_edge_support
// runs it on the device (a wavefront per tile, lane = position).  A contribution goes to the counter of the inline slot that holds its target (agx_support_slot), else —
// sources with AGX_NF_EOVF — to the first entry of the overflow list that names the pair (agx_support_ovf_entry), else to `unmatched`: the kernel's rule, in plain adds.
// tests/test_edge_support_cases.py compiles this into a shared library with g++, lays the oracle's node and edge tables out as the device's (slots = canonical ids) and
// compares the counts with tests/edge_support_model.py.
//   single_ok != 0: positions with one variant on both sides skip the resolve (the kernel's form); 0: they go through the candidate keys like every other position.
//   out[0] events, out[1] contributions, out[2] unmatched (a contribution without an edge, an event that met an index outside the tables, a list entry without a hit).
#include <stdint.h>
#include <string.h>
#include "../aligngraph_amd/csrc/agx_core.h"

extern "C" int agx_edge_support_shim(const uint32_t *cm_start, const agx_cmkey *cm, const agx_dhit *dhit, uint32_t n_hits, const agx_run *runs,
                                     const uint32_t *tile_off, const uint32_t *tile_hit, uint32_t n_pos, uint32_t k, int iv,
                                     const uint32_t *node_start, const uint16_t *node_cnt, const uint32_t *nk /* [5][pool_cap]: cid, coff, cid0, coff0, off0 */, uint32_t pool_cap,
                                     const uint32_t *n_next, const uint8_t *n_flags, const agx_edge_ovf *ovf, uint32_t n_ovf, int single_ok,
                                     uint32_t *e_cnt, uint32_t *ovf_cnt, uint64_t *out) {
    agx_sweep_args A; memset(&A, 0, sizeof A);
    A.cm_start = cm_start; A.cm = cm; A.dhit = dhit; A.runs = runs; A.tile_off = tile_off; A.n_pos = n_pos; A.n_tiles = (n_pos + AGX_TILE - 1) / AGX_TILE; A.k = k; A.iv = iv;
    A.node_start = const_cast<uint32_t *>(node_start); A.node_cnt = const_cast<uint16_t *>(node_cnt); A.pool_cap = pool_cap;
    A.nk_cid = const_cast<uint32_t *>(nk); A.nk_coff = const_cast<uint32_t *>(nk + pool_cap); A.nk_cid0 = const_cast<uint32_t *>(nk + 2 * (size_t)pool_cap);
    A.nk_coff0 = const_cast<uint32_t *>(nk + 3 * (size_t)pool_cap); A.nk_off0 = const_cast<uint32_t *>(nk + 4 * (size_t)pool_cap);
    A.n_next = const_cast<uint32_t *>(n_next); A.n_flags = const_cast<uint8_t *>(n_flags);
    uint64_t events = 0, adds = 0, unmatched = 0;
    for (uint32_t tile = 0; tile < A.n_tiles; tile++)
        for (uint32_t i = tile_off[tile]; i < tile_off[tile + 1]; i++) {
            const uint32_t hit = tile_hit[i];
            if (hit >= n_hits) { unmatched++; continue; }
            for (uint32_t lane = 0; lane < AGX_TILE; lane++) {
                bool bad = false;
                events += agx_support_lane(A, tile * AGX_TILE + lane, dhit[hit], single_ok != 0, &bad, [&](agx_u32 src, agx_u32 dst) {
                    adds++;
                    const agx_u32 e = agx_support_slot(n_next, src, dst);
                    if (e < AGX_MAXE) { e_cnt[(size_t)src * AGX_MAXE + e]++; return; }
                    const agx_u32 at = (n_flags[src] & AGX_NF_EOVF) ? agx_support_ovf_entry(ovf, n_ovf, src, dst) : n_ovf;
                    if (at < n_ovf) ovf_cnt[at]++; else unmatched++;
                });
                unmatched += bad ? 1u : 0u;
            }
        }
    out[0] = events; out[1] = adds; out[2] = unmatched;
    return 0;
}
