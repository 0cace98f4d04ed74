// agx_gfa.cpp — GFA 1.0 text of a unit's unitigs (agx_unitigs_gfa).  Host only: needs no device.
//
//   S	u<unit>_<pos>_<var>	<sequence>	LN:i:<nodes>	KC:i:<coverage>	pe:i:<last position>
//   L	<from segment>	+	<to segment>	+	0M      (agx_unitigs_gfa_support: + RC:i:<events that name the link's edge>)
//   P	p<unit>_<record>_<first base>	<segment>+,<segment>+,...	*	ln:i:<nodes>	fs:i:<first rank>	ls:i:<last rank>      (agx_unitigs_paths_gfa)
//
// S lines in segment order, then L lines in link order (agx_unit_unitigs leaves both sorted).  A large unit is formatted by several threads, each
// taking a stretch of segments and a stretch of links; the stretches are joined in order, so the text does not depend on the thread count.
#include <algorithm>
#include <charconv>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "agx_host.h"

using namespace agx;

namespace {

void put_u64(std::string &o, uint64_t v) { char b[24]; const auto r = std::to_chars(b, b + sizeof b, v); o.append(b, r.ptr); }
void put_name(std::string &o, const std::string &prefix, const agx_unitigs *t, uint32_t s) { o += prefix; put_u64(o, t->head_pos[s]); o += '_'; put_u64(o, t->head_var[s]); }

void format_segments(const agx_unitigs *t, const std::string &prefix, uint32_t lo, uint32_t hi, std::string &o) {
    size_t want = 0;
    for (uint32_t s = lo; s < hi; s++) want += 64 + (size_t)(t->seq_off[s + 1] - t->seq_off[s]);
    o.reserve(want);
    for (uint32_t s = lo; s < hi; s++) {
        o += "S\t"; put_name(o, prefix, t, s); o += '\t';
        o.append(t->seq + t->seq_off[s], (size_t)(t->seq_off[s + 1] - t->seq_off[s]));
        o += "\tLN:i:"; put_u64(o, t->n_nodes[s]); o += "\tKC:i:"; put_u64(o, t->coverage[s]); o += "\tpe:i:"; put_u64(o, t->last_pos[s]); o += '\n';
    }
}

// sup: the links' support for the RC tag, or nullptr for the line without it
void format_links(const agx_unitigs *t, const uint32_t *sup, const std::string &prefix, uint32_t lo, uint32_t hi, std::string &o) {
    o.reserve((size_t)(hi - lo) * (sup ? 72 : 56));
    for (uint32_t i = lo; i < hi; i++) {
        o += "L\t"; put_name(o, prefix, t, t->link_from[i]); o += "\t+\t"; put_name(o, prefix, t, t->link_to[i]); o += "\t+\t0M";
        if (sup) { o += "\tRC:i:"; put_u64(o, sup[i]); }
        o += '\n';
    }
}

// AGX_GFA_THREADS overrides (tests compare the text of one thread with that of many); otherwise one thread per 4 MB of expected text, at most the CPUs this process may use
unsigned gfa_threads(size_t bytes) {
    if (const char *e = getenv("AGX_GFA_THREADS")) { const int n = atoi(e); if (n >= 1) return (unsigned)std::min(n, 256); }
    const size_t by_size = bytes / (4u << 20) + 1;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(by_size, usable_cpus()));
}

// the table must describe itself: offsets non-decreasing and within n_bases, a segment's node count its stretch of bases, links between segments
bool table_ok(const agx_unitigs *t) {
    const uint32_t ns = t->n_segs, nl = t->n_links;
    if (ns && (!t->head_pos || !t->head_var || !t->n_nodes || !t->last_pos || !t->coverage || !t->seq_off)) return false;
    if (nl && (!t->link_from || !t->link_to || !ns)) return false;
    if (ns) {
        for (uint32_t s = 0; s < ns; s++)
            if (t->seq_off[s + 1] < t->seq_off[s] || t->seq_off[s + 1] - t->seq_off[s] != t->n_nodes[s]) return false;
        if (t->seq_off[ns] > t->n_bases || (t->seq_off[ns] > t->seq_off[0] && !t->seq)) return false;
    }
    for (uint32_t i = 0; i < nl; i++) if (t->link_from[i] >= ns || t->link_to[i] >= ns) return false;
    return true;
}

// One record's nodes laid over the segments: the open path, closed into a P line when the next node does not continue it
struct PathWriter {
    const agx_unitigs *t; const std::string &seg_prefix, &path_prefix; const std::vector<uint64_t> &links; std::string &o;
    bool open = false; uint32_t rec = 0, seg = 0, rank = 0, fs = 0; uint64_t first_base = 0, nodes = 0; std::string segs;
    PathWriter(const agx_unitigs *table, const std::string &sp, const std::string &pp, const std::vector<uint64_t> &l, std::string &out) : t(table), seg_prefix(sp), path_prefix(pp), links(l), o(out) {}
    void close() {
        if (!open) return;
        o += "P\t"; o += path_prefix; put_u64(o, rec); o += '_'; put_u64(o, first_base); o += '\t'; o += segs;
        o += "\t*\tln:i:"; put_u64(o, nodes); o += "\tfs:i:"; put_u64(o, fs); o += "\tls:i:"; put_u64(o, rank); o += '\n';
        open = false; segs.clear();
    }
    void visit(uint32_t s) { if (!segs.empty()) segs += ','; put_name(segs, seg_prefix, t, s); segs += '+'; }
    // n nodes of segment s from rank k on, the first one at base `base` of record r; cont: the first one follows the open path's last node (over an edge of the walk).
    // false: the pair is neither (same segment, rank + 1) nor (a segment's last node -> rank 0 of the next over a link of the table)
    bool add(uint32_t r, uint64_t base, uint32_t s, uint32_t k, uint32_t n, bool cont) {
        if (open && cont) {
            if (s == seg && k == rank + 1u) { rank = k + n - 1u; nodes += n; return true; }
            if (rank + 1u != t->n_nodes[seg] || k != 0u || !std::binary_search(links.begin(), links.end(), ((uint64_t)seg << 32) | s)) return false;
            visit(s); seg = s; rank = k + n - 1u; nodes += n;
            return true;
        }
        close();
        open = true; rec = r; first_base = base; fs = k; nodes = n; seg = s; rank = k + n - 1u; visit(s);
        return true;
    }
};

// a finished text into the caller's hands: malloc'd and terminated (agx_text_free)
int give_text(const std::string &o, char **text, size_t *len) {
    char *out = (char *)malloc(o.size() + 1);
    if (!out) return AGX_E_ARG;
    memcpy(out, o.data(), o.size()); out[o.size()] = 0;
    *text = out; *len = o.size();
    return AGX_OK;
}

}  // namespace

extern "C" {

int agx_unitigs_paths_gfa(const agx_unitigs *t, const agx_idmap *m, const agx_walk_paths *w, int unit, char **text, size_t *len) {
    if (!t || !m || !w || !text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    if (!table_ok(t)) return AGX_E_ARG;
    const uint32_t ns = t->n_segs, nr = m->n_runs;
    if (nr && (!m->id_first || !m->id_last || !m->seg || !m->rank_first)) return AGX_E_ARG;
    if (w->n_recs && (!w->rec_len || !w->st_off)) return AGX_E_ARG;
    if (w->n_stretches && (!w->id_first || !w->id_last || !w->base_off || !w->joined || !w->n_recs)) return AGX_E_ARG;
    // the map: runs in id order, main ids or side ids, inside their segments
    for (uint32_t r = 0; r < nr; r++) {
        const uint32_t a = m->id_first[r], b = m->id_last[r];
        if (a > b || b >= m->n_ids || (a < m->n_pos) != (b < m->n_pos) || (r && m->id_last[r - 1] >= a) || m->seg[r] >= ns) return AGX_E_ARG;
        if ((uint64_t)m->rank_first[r] + (b - a) >= t->n_nodes[m->seg[r]]) return AGX_E_ARG;
    }
    try {
        std::vector<uint64_t> links(t->n_links);
        for (uint32_t i = 0; i < t->n_links; i++) links[i] = ((uint64_t)t->link_from[i] << 32) | t->link_to[i];
        std::sort(links.begin(), links.end());
        const std::string seg_prefix = "u" + std::to_string(unit) + "_", path_prefix = "p" + std::to_string(unit) + "_";
        std::string o;
        PathWriter pw(t, seg_prefix, path_prefix, links, o);
        if (w->n_recs && (w->st_off[0] != 0 || w->st_off[w->n_recs] != w->n_stretches)) return AGX_E_ARG;
        for (uint32_t r = 0; r < w->n_recs; r++) {
            if (w->st_off[r] > w->st_off[r + 1]) return AGX_E_ARG;
            bool prev_end_mapped = false;      // the last id of the stretch in front is in the map
            for (uint64_t i = w->st_off[r]; i < w->st_off[r + 1]; i++) {
                const uint32_t a = w->id_first[i], b = w->id_last[i];
                if (a > b || b >= m->n_ids || (a < m->n_pos) != (b < m->n_pos) || w->base_off[i] + ((uint64_t)b - a + 1) > w->rec_len[r]) return AGX_E_ARG;
                const bool joined = w->joined[i] != 0;
                if (i == w->st_off[r] ? joined : (w->base_off[i] < w->base_off[i - 1] + ((uint64_t)w->id_last[i - 1] - w->id_first[i - 1] + 1) ||
                                                  joined != (w->base_off[i] == w->base_off[i - 1] + ((uint64_t)w->id_last[i - 1] - w->id_first[i - 1] + 1)))) return AGX_E_ARG;
                // the runs that meet [a, b]: from the first one that ends at or behind a
                uint32_t q = (uint32_t)(std::lower_bound(m->id_last, m->id_last + nr, a) - m->id_last);
                uint32_t at = a;               // the next id of the stretch to be placed
                bool cont = joined && prev_end_mapped;
                for (; q < nr && m->id_first[q] <= b; q++) {
                    const uint32_t lo = std::max(a, m->id_first[q]), hi = std::min(b, m->id_last[q]);
                    if (lo != at) cont = false;               // ids without a node in the export in between
                    if (!pw.add(r, w->base_off[i] + (lo - a), m->seg[q], m->rank_first[q] + (lo - m->id_first[q]), hi - lo + 1u, cont)) return AGX_E_ARG;
                    at = hi + 1u; cont = true;
                    if (hi == b) break;
                }
                prev_end_mapped = at == b + 1u && at != a;
                if (!prev_end_mapped) pw.close();
            }
            pw.close();
        }
        return give_text(o, text, len);
    } catch (...) {
        return AGX_E_ARG;
    }
}

void agx_unitigs_free(agx_unitigs *t) {
    if (!t) return;
    free(t->head_pos); free(t->head_var); free(t->n_nodes); free(t->last_pos); free(t->coverage); free(t->seq_off); free(t->seq); free(t->link_from); free(t->link_to);
    memset(t, 0, sizeof *t);
}

void agx_text_free(char *text) { free(text); }

// the S and L lines of either form (sup: see format_links)
static int gfa_text(const agx_unitigs *t, const uint32_t *sup, int unit, char **text, size_t *len) {
    if (!t || !text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    const uint32_t ns = t->n_segs, nl = t->n_links;
    if (!table_ok(t)) return AGX_E_ARG;
    try {
        const std::string prefix = "u" + std::to_string(unit) + "_";
        const size_t bases = ns ? (size_t)(t->seq_off[ns] - t->seq_off[0]) : 0, bytes = bases + (size_t)ns * 64 + (size_t)nl * 56;
        const unsigned nt = gfa_threads(bytes);
        // segment stretches of about equal text, link stretches of equal count
        std::vector<uint32_t> sb(nt + 1, ns), lb(nt + 1, nl);
        sb[0] = 0; lb[0] = 0;
        {   uint32_t s = 0;
            for (unsigned k = 1; k < nt; k++) {
                const size_t goal = bytes ? (size_t)((double)(bases + (size_t)ns * 64) * k / nt) : 0;
                while (s < ns && (size_t)(t->seq_off[s] - t->seq_off[0]) + (size_t)s * 64 < goal) s++;
                sb[k] = s; lb[k] = (uint32_t)((uint64_t)nl * k / nt);
            }
        }
        std::vector<std::string> so(nt), lo(nt);
        auto work = [&](unsigned k) { format_segments(t, prefix, sb[k], sb[k + 1], so[k]); format_links(t, sup, prefix, lb[k], lb[k + 1], lo[k]); };
        if (nt == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (unsigned k = 1; k < nt; k++) th.emplace_back(work, k);
            work(0);
            for (auto &x : th) x.join();
        }
        size_t n = 0;
        for (unsigned k = 0; k < nt; k++) n += so[k].size() + lo[k].size();
        char *out = (char *)malloc(n + 1);
        if (!out) return AGX_E_ARG;
        size_t at = 0;
        for (unsigned k = 0; k < nt; k++) { memcpy(out + at, so[k].data(), so[k].size()); at += so[k].size(); }
        for (unsigned k = 0; k < nt; k++) { memcpy(out + at, lo[k].data(), lo[k].size()); at += lo[k].size(); }
        out[n] = 0;
        *text = out; *len = n;
        return AGX_OK;
    } catch (...) {
        return AGX_E_ARG;
    }
}

int agx_unitigs_gfa(const agx_unitigs *t, int unit, char **text, size_t *len) { return gfa_text(t, nullptr, unit, text, len); }

int agx_unitigs_gfa_support(const agx_unitigs *t, const uint32_t *link_support, int unit, char **text, size_t *len) {
    if (text) *text = nullptr;
    if (len) *len = 0;
    if (!link_support) return AGX_E_ARG;
    return gfa_text(t, link_support, unit, text, len);
}

// An interval table as BED, one line per interval in the table's order (the weak intervals of §14, the thin ones of §16):
//   p<unit>_<rec>	<base_first>	<base_last + 1>	<label>	0	+	<tag_a><min_a>	<tag_b><min_b>      ("." for a number that is 0xFFFFFFFF)
static int intervals_bed(uint32_t n, uint32_t n_recs, const uint32_t *rec, const uint32_t *first, const uint32_t *last, const uint32_t *min_a, const uint32_t *min_b,
                         const char *label, const char *tag_a, const char *tag_b, int unit, char **text, size_t *len) {
    if (!text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    if (n && (!rec || !first || !last || !min_a || !min_b)) return AGX_E_ARG;
    for (uint32_t i = 0; i < n; i++) if (last[i] < first[i] || rec[i] >= n_recs) return AGX_E_ARG;
    try {
        const std::string prefix = "p" + std::to_string(unit) + "_";
        std::string o;
        o.reserve((size_t)n * 64);
        auto put_or_dot = [&](uint32_t v) { if (v == 0xFFFFFFFFu) o += '.'; else put_u64(o, v); };
        for (uint32_t i = 0; i < n; i++) {
            o += prefix; put_u64(o, rec[i]); o += '\t'; put_u64(o, first[i]); o += '\t'; put_u64(o, (uint64_t)last[i] + 1);
            o += '\t'; o += label; o += "\t0\t+\t"; o += tag_a; put_or_dot(min_a[i]); o += '\t'; o += tag_b; put_or_dot(min_b[i]); o += '\n';
        }
        return give_text(o, text, len);
    } catch (...) {
        return AGX_E_ARG;
    }
}

// The weak intervals of agx_unit_walk_evidence as BED:
//   p<unit>_<rec>	<base_first>	<base_last + 1>	weak	0	+	dm:i:<depth_min>	sm:i:<step_min>
int agx_walk_evidence_bed(const agx_walk_evidence *e, int unit, char **text, size_t *len) {
    if (!e) return AGX_E_ARG;
    return intervals_bed(e->n_intervals, e->n_recs, e->iv_rec, e->iv_first, e->iv_last, e->iv_depth_min, e->iv_step_min, "weak", "dm:i:", "sm:i:", unit, text, len);
}

// The thin intervals of agx_unit_walk_span as BED:
//   p<unit>_<rec>	<base_first>	<base_last + 1>	thin	0	+	pm:i:<span_min>	jm:i:<step_min>
int agx_walk_span_bed(const agx_walk_span *e, int unit, char **text, size_t *len) {
    if (!e) return AGX_E_ARG;
    return intervals_bed(e->n_intervals, e->n_recs, e->iv_rec, e->iv_first, e->iv_last, e->iv_span_min, e->iv_step_min, "thin", "pm:i:", "jm:i:", unit, text, len);
}

// The edges of agx_unit_edge_reads with the hits behind them, one line per edge in the table's order:
//   <unit>	<src_pos>	<src_var>	<dst_pos>	<dst_var>	<support>	<hit>,<hit>,...
int agx_edge_reads_tsv(const agx_edge_reads *r, int unit, char **text, size_t *len) {
    if (!r || !text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    const uint32_t n = r->n_edges;
    if (n && (!r->src_pos || !r->src_var || !r->dst_pos || !r->dst_var || !r->support || !r->hit_off)) return AGX_E_ARG;
    if (r->n_hits && !r->hit) return AGX_E_ARG;
    if (n && (r->hit_off[0] != 0 || r->hit_off[n] != r->n_hits)) return AGX_E_ARG;
    for (uint32_t i = 0; i < n; i++) if (r->hit_off[i] > r->hit_off[i + 1] || r->hit_off[i + 1] > r->n_hits) return AGX_E_ARG;
    try {
        std::string o;
        o.reserve((size_t)n * 48 + (size_t)r->n_hits * 8);
        for (uint32_t i = 0; i < n; i++) {
            put_u64(o, (uint64_t)unit); o += '\t'; put_u64(o, r->src_pos[i]); o += '\t'; put_u64(o, r->src_var[i]); o += '\t'; put_u64(o, r->dst_pos[i]); o += '\t';
            put_u64(o, r->dst_var[i]); o += '\t'; put_u64(o, r->support[i]); o += '\t';
            for (uint64_t h = r->hit_off[i]; h < r->hit_off[i + 1]; h++) { if (h != r->hit_off[i]) o += ','; put_u64(o, r->hit[h]); }
            o += '\n';
        }
        return give_text(o, text, len);
    } catch (...) {
        return AGX_E_ARG;
    }
}

// The links of agx_unit_mate_links, one line per link in the table's order, no header line:
//   p<unit>_<a>	p<unit>_<b>	<n_pairs>	<len_sum>	<lo_min>	<lo_max>	<hi_min>	<hi_max>
int agx_mate_links_tsv(const agx_mate_links *l, int unit, char **text, size_t *len) {
    if (!l || !text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    const uint32_t n = l->n_links;
    if (n && (!l->a || !l->b || !l->n_pairs || !l->len_sum || !l->lo_min || !l->lo_max || !l->hi_min || !l->hi_max)) return AGX_E_ARG;
    for (uint32_t i = 0; i < n; i++) if (l->a[i] >= l->n_recs || l->b[i] >= l->n_recs || l->a[i] == l->b[i]) return AGX_E_ARG;
    try {
        const std::string prefix = "p" + std::to_string(unit) + "_";
        std::string o;
        o.reserve((size_t)n * 64);
        for (uint32_t i = 0; i < n; i++) {
            o += prefix; put_u64(o, l->a[i]); o += '\t'; o += prefix; put_u64(o, l->b[i]); o += '\t'; put_u64(o, l->n_pairs[i]); o += '\t'; put_u64(o, l->len_sum[i]); o += '\t';
            put_u64(o, l->lo_min[i]); o += '\t'; put_u64(o, l->lo_max[i]); o += '\t'; put_u64(o, l->hi_min[i]); o += '\t'; put_u64(o, l->hi_max[i]); o += '\n';
        }
        return give_text(o, text, len);
    } catch (...) {
        return AGX_E_ARG;
    }
}

// The bubbles of an export the caller holds: the host-only twin of agx_unit_bubbles and its CPU replay.  The link offsets and in-degrees are made from the
// table, every segment is classed by agx_bubble_class — the function the kernels call —, and the rows are written as agx_k_bb_emit writes them.
int agx_unitigs_bubbles(const agx_unitigs *t, const uint32_t *link_support, uint32_t max_nodes, agx_bubbles *b) {
    if (!t || !b) return AGX_E_ARG;
    memset(b, 0, sizeof *b);
    if (!table_ok(t) || t->n_bases > 0xFFFFFFFFull) return AGX_E_ARG;
    const uint32_t ns = t->n_segs, nl = t->n_links;
    for (uint32_t i = 1; i < nl; i++) if (t->link_from[i - 1] > t->link_from[i]) return AGX_E_ARG;      // (the offsets below are those of links ordered by source)
    try {
        std::vector<agx_u32> l_off((size_t)ns + 1, 0u), s_in(ns, 0u);
        for (uint32_t i = 0; i < nl; i++) { l_off[(size_t)t->link_from[i] + 1]++; s_in[t->link_to[i]]++; }
        for (uint32_t s = 0; s < ns; s++) l_off[(size_t)s + 1] += l_off[s];
        b->n_segs = ns; b->n_links = nl; b->max_nodes = max_nodes; b->has_support = link_support ? 1u : 0u;
        std::vector<agx_bubble> cls(ns);
        uint64_t n_bub = 0, n_rows = 0, n_bases = 0;
        for (uint32_t s = 0; s < ns; s++) {
            const agx_bubble c = cls[s] = agx_bubble_class(s, l_off.data(), t->link_to, s_in.data(), t->n_nodes, ns, nl);
            if (c.cls == AGX_BB_BAD) { agx_bubbles_free(b); return AGX_E_ARG; }
            if (c.cls == AGX_BB_NONE) continue;
            b->n_forks++;
            if (c.cls == AGX_BB_TIP) b->n_tip++; else if (c.cls == AGX_BB_NESTED) b->n_nested++; else if (c.cls == AGX_BB_SINKS_DIFFER) b->n_sinks_differ++;
            else if (c.cls == AGX_BB_SINK_SHARED) b->n_sink_shared++;
            else {
                b->n_bubbles_all++; b->longest_branch = std::max(b->longest_branch, c.longest);
                if (c.longest <= max_nodes) { n_bub++; n_rows += c.k; n_bases += c.bases; }
            }
        }
        auto arr = [](size_t n, size_t sz) { void *p = calloc(n + 1, sz); if (!p) throw std::bad_alloc(); return p; };
        b->src_pos = (uint32_t *)arr(n_bub, 4); b->src_var = (uint32_t *)arr(n_bub, 4); b->src_last = (uint32_t *)arr(n_bub, 4); b->sink_pos = (uint32_t *)arr(n_bub, 4);
        b->sink_var = (uint32_t *)arr(n_bub, 4); b->br_off = (uint32_t *)arr(n_bub, 4);
        b->br_pos = (uint32_t *)arr(n_rows, 4); b->br_var = (uint32_t *)arr(n_rows, 4); b->br_nodes = (uint32_t *)arr(n_rows, 4); b->br_cov = (uint64_t *)arr(n_rows, 8);
        b->br_seq_off = (uint64_t *)arr(n_rows, 8); b->seq = (char *)arr(n_bases, 1);
        if (link_support) { b->br_sup_in = (uint32_t *)arr(n_rows, 4); b->br_sup_out = (uint32_t *)arr(n_rows, 4); }
        uint32_t at = 0, r = 0; uint64_t base = 0;
        for (uint32_t s = 0; s < ns; s++) {
            const agx_bubble &c = cls[s];
            if (c.cls != AGX_BB_BUBBLE || c.longest > max_nodes) continue;
            b->src_pos[at] = t->head_pos[s]; b->src_var[at] = t->head_var[s]; b->src_last[at] = t->last_pos[s]; b->sink_pos[at] = t->head_pos[c.sink]; b->sink_var[at] = t->head_var[c.sink];
            b->br_off[at++] = r;
            for (uint32_t i = l_off[s]; i < l_off[(size_t)s + 1]; i++, r++) {
                const uint32_t x = t->link_to[i];
                b->br_seq_off[r] = base;
                if (s_in[x] == 1u) {
                    b->br_pos[r] = t->head_pos[x]; b->br_var[r] = t->head_var[x]; b->br_nodes[r] = t->n_nodes[x]; b->br_cov[r] = t->coverage[x];
                    memcpy(b->seq + base, t->seq + t->seq_off[x], t->n_nodes[x]); base += t->n_nodes[x];
                    if (link_support) { b->br_sup_in[r] = link_support[i]; b->br_sup_out[r] = link_support[l_off[x]]; }
                } else {
                    b->br_pos[r] = b->br_var[r] = 0xFFFFFFFFu;
                    if (link_support) b->br_sup_in[r] = b->br_sup_out[r] = link_support[i];
                }
            }
        }
        b->br_off[at] = r; b->br_seq_off[r] = base;
        b->n_bubbles = at; b->n_branches = r; b->n_bases = base;
        return AGX_OK;
    } catch (...) {
        agx_bubbles_free(b);
        return AGX_E_ARG;
    }
}

void agx_bubbles_free(agx_bubbles *b) {
    if (!b) return;
    free(b->src_pos); free(b->src_var); free(b->src_last); free(b->sink_pos); free(b->sink_var); free(b->br_off);
    free(b->br_pos); free(b->br_var); free(b->br_nodes); free(b->br_cov); free(b->br_seq_off); free(b->br_sup_in); free(b->br_sup_out); free(b->seq);
    memset(b, 0, sizeof *b);
}

// The bubbles as text, one line per bubble in the table's order, no header line:
//   <source>	<sink>	<source's last position>	<sink's head position>	<k>	<names>	<nodes>	<coverage>	<support_in>	<support_out>	<bases>
// the last six as comma lists with an entry per branch; a direct branch has * for its name and bases; without support both support lists are "."
int agx_bubbles_tsv(const agx_bubbles *b, int unit, char **text, size_t *len) {
    if (!b || !text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    const uint32_t n = b->n_bubbles, nr = b->n_branches;
    if (n && (!b->src_pos || !b->src_var || !b->src_last || !b->sink_pos || !b->sink_var || !b->br_off)) return AGX_E_ARG;
    if (nr && (!b->br_pos || !b->br_var || !b->br_nodes || !b->br_cov || !b->br_seq_off || !n)) return AGX_E_ARG;
    if (b->has_support && nr && (!b->br_sup_in || !b->br_sup_out)) return AGX_E_ARG;
    if (n && (b->br_off[0] != 0 || b->br_off[n] != nr)) return AGX_E_ARG;
    for (uint32_t i = 0; i < n; i++) if (b->br_off[i] > b->br_off[i + 1] || b->br_off[i + 1] > nr) return AGX_E_ARG;
    for (uint32_t r = 0; r < nr; r++)
        if (b->br_seq_off[r] > b->br_seq_off[r + 1] || b->br_seq_off[r + 1] > b->n_bases || b->br_seq_off[r + 1] - b->br_seq_off[r] != b->br_nodes[r] || (b->br_nodes[r] && !b->seq)) return AGX_E_ARG;
    try {
        const std::string prefix = "u" + std::to_string(unit) + "_";
        std::string o;
        o.reserve((size_t)n * 64 + (size_t)nr * 48 + (size_t)b->n_bases);
        auto name = [&](uint32_t pos, uint32_t var) { o += prefix; put_u64(o, pos); o += '_'; put_u64(o, var); };
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t lo = b->br_off[i], hi = b->br_off[i + 1];
            name(b->src_pos[i], b->src_var[i]); o += '\t'; name(b->sink_pos[i], b->sink_var[i]); o += '\t'; put_u64(o, b->src_last[i]); o += '\t'; put_u64(o, b->sink_pos[i]); o += '\t';
            put_u64(o, hi - lo);
            auto list = [&](auto put) { o += '\t'; for (uint32_t r = lo; r < hi; r++) { if (r != lo) o += ','; put(r); } };
            auto direct = [&](uint32_t r) { return b->br_pos[r] == 0xFFFFFFFFu && b->br_var[r] == 0xFFFFFFFFu; };
            list([&](uint32_t r) { if (direct(r)) o += '*'; else name(b->br_pos[r], b->br_var[r]); });
            list([&](uint32_t r) { put_u64(o, b->br_nodes[r]); });
            list([&](uint32_t r) { put_u64(o, b->br_cov[r]); });
            if (b->has_support) { list([&](uint32_t r) { put_u64(o, b->br_sup_in[r]); }); list([&](uint32_t r) { put_u64(o, b->br_sup_out[r]); }); }
            else o += "\t.\t.";
            list([&](uint32_t r) { if (direct(r)) o += '*'; else o.append(b->seq + b->br_seq_off[r], (size_t)b->br_nodes[r]); });
            o += '\n';
        }
        return give_text(o, text, len);
    } catch (...) {
        return AGX_E_ARG;
    }
}

}  // extern "C"
