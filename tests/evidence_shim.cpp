// evidence_shim.cpp — TEST-ONLY: agx_evidence_lane / agx_evidence_step (csrc/agx_core.h) run serially over every flat graph base of plain arrays, and a serial replay of
// what agx_k_ev_gather / agx_k_ev_runs and the host of agx_unit_walk_evidence do with the numbers: the record sums and packed minima, per chunk the interval-start flags
// (the chunk's first base has nothing in front), their exclusive scan, the runs by interval number with their minima, and the merge of an interval cut by a chunk border.
// tests/test_evidence_cases.py compiles this with g++, lays the oracle's tables out as the device's (slots = canonical ids) and compares with tests/evidence_model.py.
//   e_cnt == nullptr: a unit without edge counters.  chunk: flat bases per chunk (a multiple of 64).
//   out[0] intervals, out[1] steps without an edge.  iv: five arrays of n_flat entries each (rec, first, last, depth_min, step_min).
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_core.h"

extern "C" int agx_evidence_shim(const uint32_t *st_first, const uint32_t *st_base, const uint32_t *st_rec, const uint32_t *st_pre, const uint8_t *st_join, uint32_t n_st, uint32_t n_flat,
                                 const uint32_t *a_nid, uint32_t n_ids, uint32_t pool_cap, const int *n_counts, const uint32_t *n_next, const uint8_t *n_flags,
                                 const agx_edge_ovf *ovf, uint32_t n_ovf, const uint32_t *e_cnt, const uint32_t *ovf_cnt,
                                 uint32_t min_depth, uint32_t min_support, uint32_t n_recs, uint32_t chunk,
                                 uint64_t *r_steps, uint64_t *r_dsum, uint64_t *r_dmin, uint64_t *r_smin, uint32_t *depth, uint32_t *votes, uint32_t *step, uint32_t *iv, uint64_t *out) {
    agx_evidence_tab T; memset(&T, 0, sizeof T);
    T.st_first = st_first; T.st_base = st_base; T.st_rec = st_rec; T.st_pre = st_pre; T.st_join = st_join; T.n_st = n_st; T.n_flat = n_flat;
    T.a_nid = a_nid; T.n_ids = n_ids; T.pool_cap = pool_cap; T.n_counts = n_counts; T.n_next = n_next; T.n_flags = n_flags; T.ovf = ovf; T.n_ovf = n_ovf; T.e_cnt = e_cnt; T.ovf_cnt = ovf_cnt;
    if (!chunk || chunk % 64u) return -1;
    for (uint32_t r = 0; r < n_recs; r++) { r_steps[r] = r_dsum[r] = 0; r_dmin[r] = r_smin[r] = ~0ull; }
    uint64_t no_edge = 0;
    std::vector<uint32_t> rec(n_flat), off(n_flat);
    for (uint32_t i = 0; i < n_flat; i++) {
        const agx_evidence_base b = agx_evidence_lane(T, i);
        if (b.st == AGX_NONE || b.rec >= n_recs) return -2;
        uint32_t s = AGX_NONE; bool ne = false;
        if (b.has_step && b.slot != AGX_NONE) {
            const uint32_t ns = agx_evidence_slot(T, b.next_id);
            if (b.inner && agx_evidence_lane(T, i + 1).slot != ns) return -3;      // (the neighbour lane's slot is the step's target where the step stays inside the stretch)
            if (ns != AGX_NONE) s = agx_evidence_step(T, b.slot, ns, &ne);
        }
        no_edge += ne ? 1 : 0;
        rec[i] = b.rec; off[i] = b.off; depth[i] = b.depth; votes[i] = b.votes; step[i] = s;
        if (s != AGX_NONE) { r_steps[b.rec]++; const uint64_t k = ((uint64_t)s << 32) | b.off; if (k < r_smin[b.rec]) r_smin[b.rec] = k; }
        if (b.depth != AGX_NONE) { r_dsum[b.rec] += b.depth; const uint64_t k = ((uint64_t)b.depth << 32) | b.off; if (k < r_dmin[b.rec]) r_dmin[b.rec] = k; }
    }
    uint32_t *iv_rec = iv, *iv_first = iv + n_flat, *iv_last = iv + 2 * (size_t)n_flat, *iv_dmin = iv + 3 * (size_t)n_flat, *iv_smin = iv + 4 * (size_t)n_flat;
    uint32_t n_iv = 0;
    for (uint64_t lo = 0; lo < n_flat; lo += chunk) {
        const uint32_t n = (uint32_t)(n_flat - lo < chunk ? n_flat - lo : chunk);
        std::vector<uint32_t> flag(n + 1, 0), foff(n + 1, 0);
        auto weak = [&](uint32_t j) { return agx_evidence_weak(depth[lo + j], step[lo + j], min_depth, min_support); };
        for (uint32_t j = 0; j < n; j++) flag[j] = weak(j) && !(j > 0 && weak(j - 1) && rec[lo + j - 1] == rec[lo + j] && off[lo + j - 1] + 1u == off[lo + j]) ? 1u : 0u;
        for (uint32_t j = 0; j < n; j++) foff[j + 1] = foff[j] + flag[j];
        const uint32_t cnt = foff[n];
        std::vector<uint32_t> c_rec(cnt), c_first(cnt), c_last(cnt), c_dmin(cnt, AGX_NONE), c_smin(cnt, AGX_NONE);
        for (uint32_t j = 0; j < n; j++) {
            if (!weak(j)) continue;
            const uint32_t r = foff[j + 1] - 1u;
            if (r >= cnt) return -4;
            if (flag[j]) { c_rec[r] = rec[lo + j]; c_first[r] = off[lo + j]; }
            if (!(j + 1 < n && weak(j + 1) && rec[lo + j + 1] == rec[lo + j] && off[lo + j + 1] == off[lo + j] + 1u)) c_last[r] = off[lo + j];
            if (depth[lo + j] < c_dmin[r]) c_dmin[r] = depth[lo + j];
            if (step[lo + j] < c_smin[r]) c_smin[r] = step[lo + j];
        }
        for (uint32_t i = 0; i < cnt; i++) {
            if (i == 0 && n_iv && iv_rec[n_iv - 1] == c_rec[0] && (uint64_t)iv_last[n_iv - 1] + 1 == c_first[0]) {
                iv_last[n_iv - 1] = c_last[0];
                if (c_dmin[0] < iv_dmin[n_iv - 1]) iv_dmin[n_iv - 1] = c_dmin[0];
                if (c_smin[0] < iv_smin[n_iv - 1]) iv_smin[n_iv - 1] = c_smin[0];
                continue;
            }
            iv_rec[n_iv] = c_rec[i]; iv_first[n_iv] = c_first[i]; iv_last[n_iv] = c_last[i]; iv_dmin[n_iv] = c_dmin[i]; iv_smin[n_iv] = c_smin[i];
            n_iv++;
        }
    }
    out[0] = n_iv; out[1] = no_edge;
    return 0;
}
