// span_shim.cpp — TEST-ONLY: the lane functions of the pair span (csrc/agx_core.h: agx_span_fragment, agx_span_clamp, agx_span_pos, agx_span_step_kind,
// agx_span_jump_walk) run serially over plain arrays, in a replay of what the kernels of agx_span.hip and the host of agx_unit_pair_span / agx_unit_walk_span do with
// them: per sub-window the mark pass, the difference, the exclusive scan and the finish; per chunk of flat bases the gather with its jump flags, their scan, the jump
// list, the host's sort and merge (agx::span_jump_entries itself, csrc/agx_host.h), the count over the hits, the scatter, the flags, their scan, the runs
// and the merge of an interval cut by a chunk border.  tests/test_span_cases.py compiles this with g++ and compares with tests/span_model.py.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_host.h"

namespace {

// one sub-window [lo, lo + n): start / end (n + 1 entries each) become span / cross; returns the three counts of the pass
void span_pass(const agx_dhit *dhit, uint32_t n_hits, const agx_run *runs, uint32_t n_runs, uint32_t n_pos, uint32_t win_lo, uint32_t win_hi, uint32_t lo, uint32_t n,
               uint32_t *start, uint32_t *end, uint64_t *counts) {
    for (uint32_t x = 0; x <= n; x++) start[x] = end[x] = 0;
    counts[0] = counts[1] = counts[2] = 0;
    for (uint32_t i = 0; i < n_hits; i++) {
        uint32_t f_lo, f_hi;
        const int kind = agx_span_fragment(dhit[i], runs, n_runs, n_pos, &f_lo, &f_hi);
        counts[1] += kind != AGX_SPAN_SKIPPED; counts[2] += kind == AGX_SPAN_OUTSIDE;
        if (kind != AGX_SPAN_FRAGMENT) continue;
        uint32_t s, e; bool has_end;
        counts[0] += agx_span_clamp(f_lo, f_hi, win_lo, win_hi, &s, &e, &has_end);
        if (agx_span_clamp(f_lo, f_hi, lo, lo + n, &s, &e, &has_end)) {
            if (s < n) start[s]++;
            if (has_end && e < n) end[e]++;
        }
    }
    for (uint32_t x = n; x-- > 1;) start[x] -= end[x - 1];                    // (agx_k_span_diff: every entry from the values before the pass)
    std::vector<uint32_t> sc(n + 1, 0);
    for (uint32_t x = 0; x < n; x++) sc[x + 1] = sc[x] + start[x];           // the exclusive scan; sc[n] the total
    for (uint32_t x = 0; x < n; x++) { const uint32_t span = sc[x + 1]; start[x] = span; end[x] = span - end[x]; }
}

}  // namespace

// span / cross of [lo, hi) in sub-windows of `sub` positions.  counts: fragments that meet the window, kept hits, outside, passes.  -1: two passes disagree.
extern "C" int agx_span_shim_pair(const agx_dhit *dhit, uint32_t n_hits, const agx_run *runs, uint32_t n_runs, uint32_t n_pos, uint32_t lo, uint32_t hi, uint32_t sub,
                                  uint32_t *span, uint32_t *cross, uint64_t *counts) {
    if (!sub || lo > hi || hi > n_pos) return -9;
    std::vector<uint32_t> start((size_t)sub + 1), end((size_t)sub + 1);
    counts[3] = 0;
    for (uint32_t x = lo; !counts[3] || x < hi;) {
        const uint32_t n = hi - x < sub ? hi - x : sub;
        uint64_t c[3];
        span_pass(dhit, n_hits, runs, n_runs, n_pos, lo, hi, x, n, start.data(), end.data(), c);
        if (counts[3] && (c[0] != counts[0] || c[1] != counts[1] || c[2] != counts[2])) return -1;
        counts[0] = c[0]; counts[1] = c[1]; counts[2] = c[2]; counts[3]++;
        for (uint32_t j = 0; j < n; j++) { span[x - lo + j] = start[j]; cross[x - lo + j] = end[j]; }
        x += n;
        if (!n) break;
    }
    return 0;
}

// The walk join.  chunk: flat bases per chunk (a multiple of 64); sub: the sub-window the unit's span and cross are made in.
//   out[0] intervals, out[1] jump steps, out[2] steps not forward, out[3] jump entries (all chunks).  iv: five arrays of n_flat entries each.
extern "C" int agx_span_shim_walk(const agx_dhit *dhit, uint32_t n_hits, const agx_run *runs, uint32_t n_runs, uint32_t n_pos, const uint32_t *side_xpos, uint32_t n_ids,
                                  const uint32_t *st_first, const uint32_t *st_base, const uint32_t *st_rec, const uint32_t *st_pre, const uint8_t *st_join, uint32_t n_st, uint32_t n_flat,
                                  uint32_t n_recs, uint32_t min_span, uint32_t chunk, uint32_t sub,
                                  uint64_t *r_steps, uint64_t *r_ssum, uint64_t *r_dmin, uint64_t *r_smin, uint32_t *pos, uint32_t *span, uint32_t *step, uint32_t *iv, uint64_t *out) {
    if (!chunk || chunk % 64u || !sub) return -9;
    std::vector<uint32_t> a_nid(n_ids ? n_ids : 1, AGX_NONE);      // (no id has a node: the pair span asks for none)
    agx_evidence_tab T; memset(&T, 0, sizeof T);
    T.st_first = st_first; T.st_base = st_base; T.st_rec = st_rec; T.st_pre = st_pre; T.st_join = st_join; T.n_st = n_st; T.n_flat = n_flat;
    T.a_nid = a_nid.data(); T.n_ids = n_ids; T.pool_cap = 0;
    // the unit's span and cross, in place as agx_unit_walk_span makes them: a sub-window's start and end are its piece of the two arrays
    std::vector<uint32_t> span_all((size_t)n_pos + 1), cross_all((size_t)n_pos + 1);
    for (uint32_t x = 0; x < n_pos; x += sub) {
        uint64_t c[3];
        span_pass(dhit, n_hits, runs, n_runs, n_pos, 0, n_pos, x, n_pos - x < sub ? n_pos - x : sub, span_all.data() + x, cross_all.data() + x, c);
    }
    for (uint32_t r = 0; r < n_recs; r++) { r_steps[r] = r_ssum[r] = 0; r_dmin[r] = r_smin[r] = ~0ull; }
    uint32_t *iv_rec = iv, *iv_first = iv + n_flat, *iv_last = iv + 2 * (size_t)n_flat, *iv_dmin = iv + 3 * (size_t)n_flat, *iv_smin = iv + 4 * (size_t)n_flat;
    uint32_t n_iv = 0;
    out[1] = out[2] = out[3] = 0;
    for (uint64_t lo = 0; lo < n_flat; lo += chunk) {
        const uint32_t n = (uint32_t)(n_flat - lo < chunk ? n_flat - lo : chunk);
        std::vector<uint32_t> rec(n), off(n), jflag(n + 1, 0), joff(n + 1, 0);
        // the gather
        for (uint32_t j = 0; j < n; j++) {
            const agx_evidence_base b = agx_evidence_lane(T, (uint32_t)lo + j);
            if (b.st == AGX_NONE || b.rec >= n_recs) return -2;
            const uint32_t x = agx_span_pos(b.id, n_pos, n_ids, side_xpos);
            uint32_t s = AGX_NONE;
            if (b.has_step) {
                const uint32_t y = agx_span_pos(b.next_id, n_pos, n_ids, side_xpos);
                if (b.inner && j + 1 < n && agx_span_pos(agx_evidence_lane(T, (uint32_t)lo + j + 1).id, n_pos, n_ids, side_xpos) != y) return -3;      // (the neighbour lane's position)
                const int kind = agx_span_step_kind(x, y);
                if (kind == AGX_SPAN_STEP_NEXT) { if (x >= n_pos) return -4; s = cross_all[x]; }
                else if (kind == AGX_SPAN_STEP_JUMP) jflag[j] = 1;
                else out[2]++;
            }
            rec[j] = b.rec; off[j] = b.off; pos[lo + j] = x; span[lo + j] = x < n_pos ? span_all[x] : AGX_NONE; step[lo + j] = s;
        }
        for (uint32_t j = 0; j < n; j++) joff[j + 1] = joff[j] + jflag[j];
        const uint32_t nj = joff[n];
        if (nj) {
            // the jump list, the host's entries, the count over the hits, the scatter
            std::vector<uint32_t> jx(nj), jy(nj), jb(nj);
            for (uint32_t j = 0; j < n; j++) {
                if (!jflag[j]) continue;
                const agx_evidence_base b = agx_evidence_lane(T, (uint32_t)lo + j);
                jx[joff[j]] = pos[lo + j]; jy[joff[j]] = agx_span_pos(b.next_id, n_pos, n_ids, side_xpos); jb[joff[j]] = (uint32_t)lo + j;
            }
            agx::SpanJumps J;
            if (!agx::span_jump_entries(jx.data(), jy.data(), jb.data(), nj, J)) return -5;
            const uint32_t ne = (uint32_t)J.e_x.size();
            for (uint32_t e = 1; e < ne; e++) if (!(J.e_x[e - 1] < J.e_x[e] || (J.e_x[e - 1] == J.e_x[e] && J.e_y[e - 1] < J.e_y[e]))) return -6;      // sorted, merged
            std::vector<uint32_t> e_cnt(ne, 0);
            for (uint32_t i = 0; i < n_hits; i++) {
                uint32_t f_lo, f_hi;
                if (agx_span_fragment(dhit[i], runs, n_runs, n_pos, &f_lo, &f_hi) == AGX_SPAN_FRAGMENT)
                    agx_span_jump_walk(J.e_x.data(), J.e_y.data(), ne, f_lo, f_hi, [&](uint32_t e) { e_cnt[e]++; });
            }
            for (uint32_t k = 0; k < nj; k++) {
                const uint32_t fb = J.l_base[k], e = J.l_ent[k];
                if (e >= ne || fb < lo || fb - lo >= n || !jflag[fb - lo]) return -7;
                step[fb] = e_cnt[e];
            }
            out[1] += nj; out[3] += ne;
        }
        // the flags, the record summaries, the runs
        std::vector<uint32_t> flag(n + 1, 0), foff(n + 1, 0);
        auto weak = [&](uint32_t j) { return agx_evidence_weak(span[lo + j], step[lo + j], min_span, min_span); };
        for (uint32_t j = 0; j < n; j++) {
            flag[j] = weak(j) && !(j > 0 && weak(j - 1) && rec[j - 1] == rec[j] && off[j - 1] + 1u == off[j]) ? 1u : 0u;
            const uint32_t r = rec[j], d = span[lo + j], s = step[lo + j];
            if (s != AGX_NONE) { r_steps[r]++; const uint64_t k = ((uint64_t)s << 32) | off[j]; if (k < r_smin[r]) r_smin[r] = k; }
            if (d != AGX_NONE) { r_ssum[r] += d; const uint64_t k = ((uint64_t)d << 32) | off[j]; if (k < r_dmin[r]) r_dmin[r] = k; }
        }
        for (uint32_t j = 0; j < n; j++) foff[j + 1] = foff[j] + flag[j];
        const uint32_t cnt = foff[n];
        std::vector<uint32_t> c_rec(cnt), c_first(cnt), c_last(cnt), c_dmin(cnt, AGX_NONE), c_smin(cnt, AGX_NONE);
        for (uint32_t j = 0; j < n; j++) {
            if (!weak(j)) continue;
            const uint32_t r = foff[j + 1] - 1u;
            if (r >= cnt) return -8;
            if (flag[j]) { c_rec[r] = rec[j]; c_first[r] = off[j]; }
            if (!(j + 1 < n && weak(j + 1) && rec[j + 1] == rec[j] && off[j + 1] == off[j] + 1u)) c_last[r] = off[j];
            if (span[lo + j] < c_dmin[r]) c_dmin[r] = span[lo + j];
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
    out[0] = n_iv;
    return 0;
}
