// links_shim.cpp — TEST-ONLY: the lane functions of the mate links (csrc/agx_core.h: agx_links_class, agx_links_key, agx_links_hash, agx_links_insert, with
// agx_span_fragment, agx_span_pos and agx_evidence_lane) run serially over plain arrays, in a replay of what the kernels of agx_links.hip and the host of
// agx_unit_mate_links do with them: init, own, shadow, the pass over all hits, the flags, their scan and the emit, under the host's range-halving loop
// (agx::links_plan itself, csrc/agx_host.h) and its sort.  tests/test_links_cases.py compiles this with g++ and compares with tests/links_model.py.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../aligngraph_amd/csrc/agx_host.h"

extern "C" uint32_t agx_links_shim_hash(uint64_t key, uint32_t log2_slots) { return agx_links_hash(key, log2_slots); }

// totals: 0 kept, 1 outside, 2 unowned, 3 inside, 4 open, 5 link pairs, 6 owned, 7 shadowed, 8 distinct keys, 9 passes, 10 links in the table, 11 passes over one record,
//         12 the probes of all inserts beyond their home slots.  rec: [5 * n_recs].  own: [n_pos].  l_key / l_len: [cap], l_num: [5 * cap] (n_pairs and the four extents).
// 0: done; -1: a single record's links do not fit (totals[9] = the record); -2 .. : the replay met something the engine calls an internal error; -9: bad arguments
extern "C" int agx_links_shim(const agx_dhit *dhit, uint32_t n_hits, const agx_run *runs, uint32_t n_runs, uint32_t n_pos, const uint32_t *side_xpos, uint32_t n_ids,
                              const uint32_t *st_first, const uint32_t *st_base, const uint32_t *st_rec, const uint32_t *st_pre, const uint8_t *st_join, uint32_t n_st, uint32_t n_flat,
                              uint32_t n_recs, uint32_t min_pairs, uint32_t slots, uint64_t *totals, uint32_t *rec, uint32_t *own, uint64_t *l_key, uint64_t *l_len, uint32_t *l_num,
                              uint32_t cap) {
    if (slots < 2 || (slots & (slots - 1u))) return -9;
    uint32_t log2_slots = 0; while ((1u << log2_slots) < slots) log2_slots++;
    std::vector<uint32_t> a_nid(n_ids ? n_ids : 1, AGX_NONE);      // (no id has a node: the links ask for none)
    agx_evidence_tab T; memset(&T, 0, sizeof T);
    T.st_first = st_first; T.st_base = st_base; T.st_rec = st_rec; T.st_pre = st_pre; T.st_join = st_join; T.n_st = n_st; T.n_flat = n_flat;
    T.a_nid = a_nid.data(); T.n_ids = n_ids; T.pool_cap = 0;
    for (int k = 0; k < 13; k++) totals[k] = 0;
    std::vector<uint64_t> t_key(slots), t_len(slots); std::vector<uint32_t> t_n(slots), t_lo_min(slots), t_lo_max(slots), t_hi_min(slots), t_hi_max(slots);
    std::vector<uint64_t> keys, lens; std::vector<uint32_t> nums[5];
    int err = 0;
    uint32_t stuck = 0;
    const long passes = agx::links_plan(n_recs, [&](uint32_t a_lo, uint32_t a_hi, bool first) {
        // agx_k_ln_init
        if (first) { for (uint32_t x = 0; x < n_pos; x++) own[x] = AGX_NONE; for (size_t i = 0; i < 5 * (size_t)n_recs; i++) rec[i] = 0; }
        for (uint32_t s = 0; s < slots; s++) { t_key[s] = AGX_LINKS_EMPTY; t_len[s] = 0; t_n[s] = 0; t_lo_min[s] = AGX_NONE; t_lo_max[s] = 0; t_hi_min[s] = AGX_NONE; t_hi_max[s] = 0; }
        if (first) {
            // agx_k_ln_own, agx_k_ln_shadow
            for (uint32_t i = 0; i < n_flat; i++) {
                const agx_evidence_base b = agx_evidence_lane(T, i);
                if (b.st == AGX_NONE || b.rec >= n_recs) { err = -2; continue; }
                const uint32_t x = agx_span_pos(b.id, n_pos, n_ids, side_xpos);
                if (x < n_pos && b.rec < own[x]) own[x] = b.rec;
            }
            for (uint32_t i = 0; i < n_flat; i++) {
                const agx_evidence_base b = agx_evidence_lane(T, i);
                if (b.st == AGX_NONE || b.rec >= n_recs) continue;
                const uint32_t x = agx_span_pos(b.id, n_pos, n_ids, side_xpos);
                if (x < n_pos && own[x] != b.rec) totals[7]++;
            }
            for (uint32_t x = 0; x < n_pos; x++) totals[6] += own[x] != AGX_NONE;
        }
        // agx_k_ln_pass
        uint64_t dropped = 0;
        for (uint32_t i = 0; i < n_hits; i++) {
            uint32_t f_lo, f_hi;
            const int kind = agx_span_fragment(dhit[i], runs, n_runs, n_pos, &f_lo, &f_hi);
            if (first) { totals[0] += kind != AGX_SPAN_SKIPPED; totals[1] += kind == AGX_SPAN_OUTSIDE; }
            if (kind != AGX_SPAN_FRAGMENT) continue;
            const uint32_t a = f_lo < n_pos ? own[f_lo] : AGX_NONE, b = f_hi < n_pos ? own[f_hi] : AGX_NONE;
            if ((a != AGX_NONE && a >= n_recs) || (b != AGX_NONE && b >= n_recs)) { err = -3; continue; }
            const int cls = agx_links_class(a, b);
            if (first) {
                if (cls == AGX_LINKS_UNOWNED) totals[2]++;
                else if (cls == AGX_LINKS_INSIDE) { totals[3]++; rec[a]++; }
                else if (cls == AGX_LINKS_OPEN_LEFT) { totals[4]++; rec[(size_t)n_recs + b]++; }
                else if (cls == AGX_LINKS_OPEN_RIGHT) { totals[4]++; rec[2 * (size_t)n_recs + a]++; }
                else { totals[5]++; rec[3 * (size_t)n_recs + a]++; rec[4 * (size_t)n_recs + b]++; }
            }
            if (cls == AGX_LINKS_LINK && a >= a_lo && a < a_hi) {
                const uint64_t key = agx_links_key(a, b);
                const uint32_t home = agx_links_hash(key, log2_slots) & (slots - 1u);
                agx_links_insert(key, slots, log2_slots,
                    [&](uint32_t s, unsigned long long k) { const uint64_t was = t_key[s]; if (was == AGX_LINKS_EMPTY) t_key[s] = k; return (unsigned long long)was; },
                    [&](uint32_t s) {
                        t_n[s]++; t_len[s] += (uint64_t)(f_hi - f_lo) + 1u;
                        t_lo_min[s] = std::min(t_lo_min[s], f_lo); t_lo_max[s] = std::max(t_lo_max[s], f_lo); t_hi_min[s] = std::min(t_hi_min[s], f_hi); t_hi_max[s] = std::max(t_hi_max[s], f_hi);
                        totals[12] += (s - home) & (slots - 1u);
                    },
                    [&]() { dropped++; });
            }
        }
        if (a_hi - a_lo <= 1u) totals[11]++;
        if (dropped) return false;      // the pass is discarded
        // agx_k_ln_flag, the scan, agx_k_ln_emit
        std::vector<uint32_t> flag(slots + 1, 0), off(slots + 1, 0);
        for (uint32_t s = 0; s < slots; s++) { const bool used = t_key[s] != AGX_LINKS_EMPTY; totals[8] += used; flag[s] = used && t_n[s] >= min_pairs; }
        for (uint32_t s = 0; s < slots; s++) off[s + 1] = off[s] + flag[s];
        for (uint32_t s = 0; s < slots; s++) {
            if (!flag[s]) continue;
            keys.push_back(t_key[s]); lens.push_back(t_len[s]);
            const uint32_t v[5] = {t_n[s], t_lo_min[s], t_lo_max[s], t_hi_min[s], t_hi_max[s]};
            for (int k = 0; k < 5; k++) nums[k].push_back(v[k]);
            if (off[s] + 1u != off[s + 1]) err = -4;
        }
        return true;
    }, &stuck);
    if (err) return err;
    if (passes < 0) { totals[9] = stuck; return -1; }
    totals[9] = (uint64_t)passes;
    if (totals[2] + totals[3] + totals[4] + totals[5] != totals[0] - totals[1]) return -5;      // the engine's identity
    const size_t nl = keys.size();
    if (nl > cap) return -6;
    std::vector<size_t> order(nl);
    for (size_t i = 0; i < nl; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    for (size_t i = 1; i < nl; i++) if (keys[order[i - 1]] == keys[order[i]]) return -7;
    for (size_t i = 0; i < nl; i++) { l_key[i] = keys[order[i]]; l_len[i] = lens[order[i]]; for (int k = 0; k < 5; k++) l_num[(size_t)k * cap + i] = nums[k][order[i]]; }
    totals[10] = nl;
    return 0;
}
