// agx_gfa.cpp — GFA 1.0 text of a unit's unitigs (agx_unitigs_gfa).  Host only: needs no device.
//
//   S	u<unit>_<pos>_<var>	<sequence>	LN:i:<nodes>	KC:i:<coverage>	pe:i:<last position>
//   L	<from segment>	+	<to segment>	+	0M
//
// S lines in segment order, then L lines in link order (agx_unit_unitigs leaves both sorted).  A large unit is formatted by several threads, each
// taking a stretch of segments and a stretch of links; the stretches are joined in order, so the text does not depend on the thread count.
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

void format_links(const agx_unitigs *t, const std::string &prefix, uint32_t lo, uint32_t hi, std::string &o) {
    o.reserve((size_t)(hi - lo) * 56);
    for (uint32_t i = lo; i < hi; i++) {
        o += "L\t"; put_name(o, prefix, t, t->link_from[i]); o += "\t+\t"; put_name(o, prefix, t, t->link_to[i]); o += "\t+\t0M\n";
    }
}

// AGX_GFA_THREADS overrides (tests compare the text of one thread with that of many); otherwise one thread per 4 MB of expected text, at most the CPUs this process may use
unsigned gfa_threads(size_t bytes) {
    if (const char *e = getenv("AGX_GFA_THREADS")) { const int n = atoi(e); if (n >= 1) return (unsigned)std::min(n, 256); }
    const size_t by_size = bytes / (4u << 20) + 1;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(by_size, usable_cpus()));
}

}  // namespace

extern "C" {

void agx_unitigs_free(agx_unitigs *t) {
    if (!t) return;
    free(t->head_pos); free(t->head_var); free(t->n_nodes); free(t->last_pos); free(t->coverage); free(t->seq_off); free(t->seq); free(t->link_from); free(t->link_to);
    memset(t, 0, sizeof *t);
}

void agx_text_free(char *text) { free(text); }

int agx_unitigs_gfa(const agx_unitigs *t, int unit, char **text, size_t *len) {
    if (!t || !text || !len || unit < 0) return AGX_E_ARG;
    *text = nullptr; *len = 0;
    const uint32_t ns = t->n_segs, nl = t->n_links;
    if (ns && (!t->head_pos || !t->head_var || !t->n_nodes || !t->last_pos || !t->coverage || !t->seq_off)) return AGX_E_ARG;
    if (nl && (!t->link_from || !t->link_to || !ns)) return AGX_E_ARG;
    // the table must describe itself: offsets non-decreasing and within n_bases, a segment's node count its stretch of bases, links between segments
    if (ns) {
        for (uint32_t s = 0; s < ns; s++)
            if (t->seq_off[s + 1] < t->seq_off[s] || t->seq_off[s + 1] - t->seq_off[s] != t->n_nodes[s]) return AGX_E_ARG;
        if (t->seq_off[ns] > t->n_bases || (t->seq_off[ns] > t->seq_off[0] && !t->seq)) return AGX_E_ARG;
    }
    for (uint32_t i = 0; i < nl; i++) if (t->link_from[i] >= ns || t->link_to[i] >= ns) return AGX_E_ARG;
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
        auto work = [&](unsigned k) { format_segments(t, prefix, sb[k], sb[k + 1], so[k]); format_links(t, prefix, lb[k], lb[k + 1], lo[k]); };
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

}  // extern "C"
