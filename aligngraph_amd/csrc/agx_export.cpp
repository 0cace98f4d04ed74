// agx_export.cpp — the calls that answer a question about a built unit on request, out of the scratch the unit's block reserves for them (d_ut) and on a stream of their
// own: the layouts that carve that buffer, Export and ensure_support, the unitig exports, edge support, edge reads, the walk's stretch table (FlatTable), the evidence and
// the pair span under its records (records_body), pair span, mate links and bubbles.  None touches the build path: that, and the calls that copy build state out, is agx_engine.cpp.
#include "agx_unit.h"

namespace agx {

// Carves the export layouts below out of one buffer: every array at the next multiple of 256 bytes, an empty one as one element; base == nullptr: only the size
struct Carve {
    char *base; size_t at = 0;
    template <class T> void operator()(T *&p, size_t n) { at = (at + 255) & ~(size_t)255; p = base ? (T *)(base + at) : nullptr; at += (n ? n : 1) * sizeof(T); }
    size_t bytes() const { return at + 256; }
};
// words of block sums that agx_launch_exclusive_scan's two levels take for n entries at `block` entries per workgroup (the callers add their slack)
inline size_t scan_words(size_t n, size_t block) { return 2 * ((n + block - 1) / block + 1) + 2 * ((n + block * block - 1) / (block * block) + 1); }
// what three layouts below hold alike: the uploaded stretch table with its prefix, and the per-record table of the two calls under the records
inline void carve_stretches(Carve &take, agx_evidence_tab &T, size_t n_st) { take(T.st_first, n_st); take(T.st_base, n_st); take(T.st_rec, n_st); take(T.st_pre, n_st + 1); take(T.st_join, n_st + 1); }
inline void carve_records(Carve &take, agx_evidence_args &E, size_t n_recs) { take(E.r_steps, n_recs); take(E.r_dsum, n_recs); take(E.r_dmin, n_recs); take(E.r_smin, n_recs); }

// The unitig export's scratch (agx_unit_unitigs, agx_unitig.hip) as one buffer carved in this order; base == nullptr: only the size.  Sized for the worst case — every
// node slot a piece and a segment — since a unit that keeps counts has it reserved with its block (plan_capacities): an export never asks the device for memory.
// Phase 3 reuses what phases 1-2 are done with: the links lie over pos_of | outs | oout | p_len | p_next, the bases over succ.
size_t unitig_layout(size_t cap, size_t n_pos, size_t n_ovf, char *base, agx_unitig_args *A, agx_u32 **words) {
    Carve take{base};
    agx_unitig_args T{}; agx_unitig_args &X = A ? *A : T; agx_u32 *w = nullptr, *R = nullptr;
    size_t hash_n = 64; while (hash_n < 2 * n_ovf) hash_n *= 2;
    const size_t nwin = (cap + 63) / 64, nmax = std::max(std::max(cap, n_pos), nwin) + 1;
    take(w, 8); take(R, 5 * cap + n_ovf);
    take(X.indeg, cap); take(X.succ, cap); take(X.osucc, cap); take(X.nxt, cap); take(X.haspred, cap);
    take(X.ovf_hash, hash_n); take(X.ovf_first, n_ovf); take(X.wcnt, nwin + 1); take(X.woff, nwin + 1);
    for (int i = 0; i < 2; i++) { take(X.anc[i], cap); take(X.off[i], cap); }
    take(X.p_seg, cap); take(X.hcnt, n_pos + 1); take(X.hoff, n_pos + 1);
    take(X.s_len, cap + 1); take(X.s_links, cap + 1); take(X.s_hpos, cap); take(X.s_hvar, cap); take(X.s_last, cap); take(X.s_cov, cap);
    take(X.s_off, cap + 1); take(X.l_off, cap + 1); take(X.l_cur, cap + 1);
    take(X.scan_tmp, scan_words(nmax, 4096) + 8);
    if (base) {
        X.pos_of = R; X.outs = R + cap; X.oout = R + 2 * cap; X.p_len = R + 3 * cap; X.p_next = R + 4 * cap;
        X.l_to = R; X.link_cap = (agx_u32)std::min<size_t>(5 * cap + n_ovf, 0xFFFFFFFFull); X.seq = (char *)X.succ; X.seq_cap = (agx_u32)std::min<size_t>(4 * cap, 0xFFFFFFFFull);
        X.hash_mask = (agx_u32)(hash_n - 1);
        if (words) *words = w;
    }
    return take.bytes();
}

// The scratch of a region export (agx_unit_unitigs_region) carved from the front of the same buffer: `kept` nodes of `n_win` positions.  What must be in place before the
// kept count is known (the words, the reverse map, the window's counts, the scans' block sums) comes first, at offsets that do not depend on it; the rest is per kept node.
// 22 words per kept node and one per slot (the reverse map, which is written at the window's slots only) where unitig_layout takes 24 per slot, so from a few hundred
// slots on it fits the whole export's buffer.  Below that its few more 256-byte-aligned pieces can make it some hundred bytes larger: agx_unit_unitigs_region takes the
// larger of the two sizes, which then comes out of the regrowth room of the unit's own block (regrow_slack: 6.4 MB at least), never from the device.  Phase 3 reuses what phases 1-2 are done with: the links lie over outs | oout | p_len | p_next, the bases over succ, the scans of segment lengths and
// link counts and the link cursors over the pointer jumping's arrays.
size_t unitig_region_layout(size_t cap, size_t n_win, size_t kept, size_t n_ovf, char *base, agx_unitig_region_args *A, agx_u32 **words) {
    Carve take{base};
    agx_unitig_region_args T{}; agx_unitig_region_args &R = A ? *A : T; agx_unitig_args &X = R.U; agx_u32 *w = nullptr, *L = nullptr;
    size_t hash_n = 64; while (hash_n < 2 * n_ovf) hash_n *= 2;
    const size_t ngrp = (kept + 63) / 64, nmax = std::max(n_win, cap) + 1;
    take(w, 8); take(R.rmap, cap); take(R.cntw, n_win + 1); take(R.offw, n_win + 1);
    take(X.scan_tmp, scan_words(nmax, 4096) + 8);
    take(X.ovf_hash, hash_n); take(X.ovf_first, n_ovf);
    take(R.l_slot, kept); take(X.pos_of, kept); take(L, 4 * kept + n_ovf);
    take(X.indeg, kept); take(X.succ, kept); take(X.osucc, kept); take(X.nxt, kept); take(X.haspred, kept);
    take(X.wcnt, ngrp + 1); take(X.woff, ngrp + 1); take(X.hcnt, ngrp + 1); take(X.hoff, ngrp + 1);
    for (int i = 0; i < 2; i++) { take(X.anc[i], kept + 1); take(X.off[i], kept + 1); }
    take(X.p_seg, kept);
    take(X.s_len, kept + 1); take(X.s_links, kept + 1); take(X.s_hpos, kept); take(X.s_hvar, kept); take(X.s_last, kept); take(X.s_cov, kept);
    if (base) {
        X.outs = L; X.oout = L + kept; X.p_len = L + 2 * kept; X.p_next = L + 3 * kept;
        X.l_to = L; X.link_cap = (agx_u32)std::min<size_t>(4 * kept + n_ovf, 0xFFFFFFFFull); X.seq = (char *)X.succ; X.seq_cap = (agx_u32)std::min<size_t>(4 * kept, 0xFFFFFFFFull);
        X.s_off = X.anc[0]; X.l_off = X.off[0]; X.l_cur = X.anc[1];
        X.hash_mask = (agx_u32)(hash_n - 1);
        if (words) *words = w;
    }
    return take.bytes();
}

// The scratch of an export's id map (agx_unit_unitigs_mapped, agx_unitig.hip: agx_k_idm_*), behind the export's own in the same buffer: `ids` window ids (the window's main
// ids and the side ids of its positions), `runs` runs at most (a run holds a kept node at least).  Two words per window id and four per run.
size_t idmap_layout(size_t ids, size_t runs, char *base, agx_idmap_args *A) {
    Carve take{base};
    agx_idmap_args T{}; agx_idmap_args &M = A ? *A : T;
    take(M.flag, ids + 1); take(M.foff, ids + 1);
    take(M.scan_tmp, scan_words(ids + 1, 1024) + 16);
    take(M.r_first, runs); take(M.r_last, runs); take(M.r_seg, runs); take(M.r_rank, runs);
    return take.bytes();
}
// The scratch of the evidence under the walk's records (agx_unit_walk_evidence, agx_evidence.hip), from the front of the same buffer: the uploaded stretch table with its
// prefix and the per-record table (the whole call's), then what one CHUNK of flat graph bases takes — depth and step per base (and votes when the tracks are wanted), the
// interval-start flags with their scan, and the chunk's intervals at their worst (every base one).  40 bytes per base of the chunk, 44 with tracks.
size_t evidence_layout(size_t n_st, size_t n_recs, size_t chunk, bool tracks, char *base, agx_evidence_args *A, agx_u32 **words) {
    Carve take{base};
    agx_evidence_args T{}; agx_evidence_args &E = A ? *A : T; agx_u32 *w = nullptr;
    take(w, 8);
    carve_stretches(take, E.T, n_st); carve_records(take, E, n_recs);
    take(E.c_depth, chunk); take(E.c_step, chunk);
    if (tracks) take(E.c_votes, chunk);
    take(E.flag, chunk + 1); take(E.foff, chunk + 1); take(E.scan_tmp, scan_words(chunk + 1, 1024) + 16);
    take(E.iv_rec, chunk); take(E.iv_first, chunk); take(E.iv_last, chunk); take(E.iv_dmin, chunk); take(E.iv_smin, chunk);
    if (base) { E.noedge = w + 1; E.err = w; if (words) *words = w; }
    return take.bytes();
}
// The scratch of the edge reads (agx_unit_edge_reads, agx_k_edge_reads), from the front of the same buffer: what one CHUNK of `tiles` tiles takes — the count per position
// with its scan (a closing entry each) and the scan's block sums — and behind it `recs` records of 16 bytes.  recs = 0: what must fit before any record does.
size_t edge_reads_layout(size_t tiles, size_t recs, char *base, agx_reads_kargs *K, agx_u32 **words) {
    Carve take{base};
    agx_reads_kargs T{}; agx_reads_kargs &R = K ? *K : T; agx_u32 *w = nullptr;
    const size_t n = tiles * AGX_TILE;
    take(w, 8); take(R.cnt, n + 1); take(R.off, n + 1); take(R.scan_tmp, scan_words(n + 1, 1024) + 16);
    take(R.recs, 4 * recs);
    if (base) { R.err = w; if (words) *words = w; }
    return take.bytes();
}
// The scratch of the pair span (agx_unit_pair_span, agx_span.hip), from the front of the same buffer: the mark pass's partials (`parts` wavefronts, three words each) and
// what one SUB-WINDOW of `sub` positions takes — start and end (span and cross in the end), the scan and its block sums, a closing entry each.  12 bytes per position.
size_t span_layout(size_t sub, size_t parts, char *base, agx_span_args *A) {
    Carve take{base};
    agx_span_args T{}; agx_span_args &S = A ? *A : T;
    take(S.part, 3 * parts); take(S.start, sub + 1); take(S.end, sub + 1); take(S.sc, sub + 1); take(S.scan_tmp, scan_words(sub + 1, 1024) + 16);
    if (base) S.n_part = (agx_u32)parts;
    return take.bytes();
}
// The scratch of the pair span under the walk's records (agx_unit_walk_span).  The whole call's: the uploaded stretch table and the per-record table as evidence_layout has
// them, the partials, and the whole unit's span and cross (8 bytes per position).  Behind that one region that serves two uses in turn: first the scan of one SUB-WINDOW
// of `sub` positions while span and cross are made (their start and end are the sub-window's piece of span and cross themselves), then what one CHUNK of flat graph bases
// takes — position, span and step per base, the jump flags and the interval-start flags with their scans, the chunk's jumps as listed, as entries and as (base, entry)
// pairs, and its intervals, each at its worst (every base a jump, every base an interval).  80 bytes per base of the chunk.
size_t walk_span_layout(size_t n_st, size_t n_recs, size_t n_pos, size_t sub, size_t chunk, size_t parts, char *base, agx_walk_span_args *A, agx_span_args *SA, agx_u32 **words) {
    Carve take{base};
    agx_walk_span_args T{}; agx_walk_span_args &W = A ? *A : T; agx_span_args TS{}; agx_span_args &S = SA ? *SA : TS;
    agx_evidence_args &E = W.E; agx_u32 *w = nullptr, *span = nullptr, *cross = nullptr, *e_x = nullptr, *e_y = nullptr, *l_base = nullptr, *l_ent = nullptr;
    take(w, 8);
    carve_stretches(take, E.T, n_st); carve_records(take, E, n_recs);
    take(S.part, 3 * parts); take(span, n_pos + 1); take(cross, n_pos + 1);
    Carve pass = take;      // the region's first use
    pass(S.sc, sub + 1); pass(S.scan_tmp, scan_words(sub + 1, 1024) + 16);
    take(W.c_pos, chunk); take(E.c_depth, chunk); take(E.c_step, chunk);
    take(W.jflag, chunk + 1); take(W.joff, chunk + 1); take(E.flag, chunk + 1); take(E.foff, chunk + 1); take(E.scan_tmp, scan_words(chunk + 1, 1024) + 16);
    take(W.jt_x, chunk); take(W.jt_y, chunk); take(W.jt_base, chunk); take(e_x, chunk); take(e_y, chunk); take(W.e_cnt, chunk); take(l_base, chunk); take(l_ent, chunk);
    take(E.iv_rec, chunk); take(E.iv_first, chunk); take(E.iv_last, chunk); take(E.iv_dmin, chunk); take(E.iv_smin, chunk);
    if (base) {
        E.noedge = w + 1; E.err = w; E.c_votes = nullptr; if (words) *words = w;
        W.span = span; W.cross = cross; W.e_x = e_x; W.e_y = e_y; W.l_base = l_base; W.l_ent = l_ent;
        S.start = span; S.end = cross; S.n_part = (agx_u32)parts;
    }
    return std::max(take.bytes(), pass.bytes());
}
// The scratch of the mate links (agx_unit_mate_links, agx_links.hip), from the front of the same buffer.  The whole call's: the uploaded stretch table as evidence_layout
// has it, own (4 bytes per position), the five per-record counters and the partials of the pass and of the shadow count.  One pass's: the table of `slots` slots as a
// structure of arrays (36 bytes per slot: key and length sum of 8, count and four extents of 4), the kept slots' flags with their scan, and the compacted output at its
// worst (every slot kept).  80 bytes per slot.
size_t links_layout(size_t n_st, size_t n_recs, size_t n_pos, size_t parts, size_t sparts, size_t slots, char *base, agx_links_args *A) {
    Carve take{base};
    agx_links_args T{}; agx_links_args &L = A ? *A : T;
    take(L.words, 8);
    carve_stretches(take, L.T, n_st);
    take(L.own, n_pos); take(L.rec, 5 * n_recs); take(L.part, 6 * parts); take(L.spart, 2 * sparts);
    take(L.t_key, slots); take(L.t_len, slots); take(L.t_n, slots); take(L.t_lo_min, slots); take(L.t_lo_max, slots); take(L.t_hi_min, slots); take(L.t_hi_max, slots);
    take(L.flag, slots + 1); take(L.off, slots + 1); take(L.scan_tmp, scan_words(slots + 1, 1024) + 16);
    take(L.o_key, slots); take(L.o_len, slots); take(L.o_n, slots); take(L.o_lo_min, slots); take(L.o_lo_max, slots); take(L.o_hi_min, slots); take(L.o_hi_max, slots);
    if (base) { L.n_part = (agx_u32)parts; L.n_spart = (agx_u32)sparts; L.out_cap = (agx_u32)slots; }
    return take.bytes();
}
// The export buffer of a unit that keeps paths: every export of such a unit takes the same size — the larger of the two export layouts at their worst, and behind it (at `map_at`)
// the id map's scratch for a whole-window map — so that exports of any kind in any order never take the buffer twice.
size_t mapped_scratch(size_t cap, size_t n_pos, size_t n_nodes, size_t n_ids, size_t n_ovf, size_t *map_at) {
    const size_t kept = std::min(n_nodes, cap), sides = n_ids > n_pos ? n_ids - n_pos : 0;
    const size_t front = (std::max(unitig_layout(cap, n_pos, n_ovf, nullptr, nullptr, nullptr), unitig_region_layout(cap, n_pos, kept, n_ovf, nullptr, nullptr, nullptr)) + 255) & ~(size_t)255;
    if (map_at) *map_at = front;
    return front + idmap_layout(n_pos + sides, std::min(kept, n_pos + sides), nullptr, nullptr);
}

// What a region export no longer reads once its phase 3 (and, on request, agx_k_utr_link_support) has run: of everything unitig_region_layout carves from l_slot on, only the
// tables themselves stay live — s_hpos, s_hvar, s_last, s_len and s_cov at `ns` segments, s_off and l_off at ns + 1, the first `nl` words of l_to and the first `nb` bytes
// of seq.  The rest is free: l_slot, pos_of, the links' room behind nl, indeg, what succ has behind the bases, osucc, nxt, haspred, the piece and head counts with their
// scans, the pointer jumping's arrays behind the two offset scans, p_seg, s_links, every per-segment array behind its ns entries, and whatever the buffer holds behind the
// layout (the id map's scratch of a unit that keeps paths: a bubble call makes no map).  Gaps lists those stretches in address order and hands arrays out of them first
// fit, each at the next multiple of 256 bytes.
struct Gaps {
    std::vector<std::pair<char *, char *> > free;
    Gaps(char *lo, char *hi, std::vector<std::pair<const void *, size_t> > live) {
        std::sort(live.begin(), live.end());
        char *at = lo;
        for (const auto &l : live) {
            char *p = (char *)const_cast<void *>(l.first);
            if (p > at) free.emplace_back(at, std::min(p, hi));
            at = std::max(at, p + l.second);
        }
        if (at < hi) free.emplace_back(at, hi);
    }
    template <class T> void operator()(T *&p, size_t n) {
        const size_t bytes = (n ? n : 1) * sizeof(T);
        for (auto &z : free) {
            char *a = (char *)(((uintptr_t)z.first + 255) & ~(uintptr_t)255);
            if (a <= z.second && bytes <= (size_t)(z.second - a)) { p = (T *)a; z.first = a + bytes; return; }
        }
        throw Error{E_UNSUPPORTED, "bubbles: the export's scratch has no " + std::to_string(bytes) + " bytes left behind the segment table"};
    }
};
// The scratch of the bubbles (agx_unit_bubbles, agx_bubbles.hip) out of those gaps, in two steps.  rows == false: what the class pass takes — the in-degrees, three
// counts and three scans per segment (a closing entry each) and the wavefronts' partials, 28 bytes per segment and 32 per wavefront.  rows == true, with the three totals
// read: the bubble rows (24 bytes each), the branch rows (40) and the bases.
void bubbles_layout(Gaps &take, bool rows, agx_bubbles_args &A) {
    if (!rows) {
        const size_t n = (size_t)A.n_segs + 1;
        take(A.tot, 8); take(A.s_in, n); take(A.flag, n); take(A.kcnt, n); take(A.bcnt, n); take(A.boff, n); take(A.koff, n); take(A.baoff, n); take(A.part, 8 * (size_t)A.n_part);
        return;
    }
    const size_t nb = A.bub_cap, nr = A.row_cap;
    take(A.b_spos, nb); take(A.b_svar, nb); take(A.b_slast, nb); take(A.b_tpos, nb); take(A.b_tvar, nb); take(A.b_broff, nb);
    take(A.r_pos, nr); take(A.r_var, nr); take(A.r_nodes, nr); take(A.r_seqoff, nr); take(A.r_seg, nr); take(A.r_in, nr); take(A.r_out, nr); take(A.r_cov, nr); take(A.o_seq, A.base_cap);
}

}  // namespace agx

namespace {

// a caller's array of n entries and a closing one, zeroed
template <class T> void host_array(T *&p, size_t n) { p = (T *)calloc(n + 1, sizeof(T)); if (!p) throw Error{E_ARG, "out of host memory"}; }

// The shape of the entry points below: no null argument (`given`: the further ones), the answer cleared, the body under `guarded`, the answer released again if it failed
template <class A, class F> int answer(agx_unit *u, A *a, void (*release)(A *), bool given, F body) {
    if (!u || !a || !given) return AGX_E_ARG;
    memset(a, 0, sizeof *a);
    const int rc = guarded(u, body);
    if (rc != AGX_OK) release(a);
    return rc;
}

}  // namespace

extern "C" {

// Unitig export: the kernels of agx_unitig.hip on a stream of the export's own, scratch from the buffer the unit's block reserves for it (d_ut).  The whole
// export (agx_unit_unitigs) and the region export (agx_unit_unitigs_region, agx_unit_unitigs_mapped) each get as far as their piece count in their own way, over slots or
// over the window's local ids; from there to the table in the caller's memory they are one body, export_body.

// what every export refuses (map: the call also makes an id map), and under its own name and in its own words the evidence under the records
static void export_check(const agx_unit *u, bool map, const std::string &who = "unitigs", const char *counts = "the segments' coverage needs the counts", const char *asked = "exports") {
    if (!(u->prm.flags & AGX_FLAG_KEEP_COUNTS)) throw Error{E_ARG, who + ": the unit was created without AGX_FLAG_KEEP_COUNTS (" + counts + ")"};
    if (!u->built || u->trimmed) throw Error{E_ARG, who + ": the unit is not built (call agx_unit_build; not after agx_unit_trim or agx_unit_release)"};
    if ((u->prm.flags & AGX_FLAG_ONE_SHOT) && (u->consumed || u->downloaded)) throw Error{E_ARG, who + ": a one-shot unit " + asked + " before its download or finish"};
    if (map && !(u->prm.flags & AGX_FLAG_KEEP_PATHS)) throw Error{E_ARG, "unitigs: the unit was created without AGX_FLAG_KEEP_PATHS (the id map's scratch is reserved with the unit's block)"};
}

// what the calls over a window of positions refuse (what: the call and its word for the window)
static void window_check(const agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, const char *what) {
    if (pos_lo > pos_hi || pos_hi > (agx_u32)u->V.n_pos)
        throw Error{E_ARG, std::string(what) + " [" + std::to_string(pos_lo) + ", " + std::to_string(pos_hi) + ") is not within the unit's positions [0, " + std::to_string((agx_u32)u->V.n_pos) + ")"};
}

// What an export holds while it runs: the unit's device with its build finished, then (open) the scratch buffer and a stream of the export's own
struct Export {
    agx_unit *u; const agx_u32 n_pos, cap, n_ovf; hipStream_t s = nullptr; size_t map_at = 0;      // map_at: where the id map's scratch begins (a unit that keeps paths)
    explicit Export(agx_unit *unit) : u(unit), n_pos((agx_u32)unit->V.n_pos), cap(unit->pool_cap), n_ovf(std::min(unit->n_ovf, unit->ovf_cap)) {
        HIP_OK(hipSetDevice(u->prm.device));
        HIP_OK(wait_event(u->ev_built));
    }
    Export(const Export &) = delete;
    ~Export() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }      // (the export's work is done before the call returns, also on an error)
    // own: what this export's layout takes — out of the room the upload reserved for it; a unit whose pool or overflow list grew takes the difference.  A unit that keeps
    // paths takes mapped_scratch whatever the export
    void open(size_t own) {
        u->d_ut.alloc(u->arena, keeps_paths(u) ? mapped_scratch(cap, n_pos, u->n_nodes, u->n_ids, n_ovf, &map_at) : own);
        u->stats.device_bytes = u->arena.capacity();
        open_stream();
    }
    void open() { open(unitig_layout(cap, n_pos, n_ovf, nullptr, nullptr, nullptr)); }      // (the buffer every export of the unit takes: the room the upload reserved)
    void open_stream() { HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }      // (alone: a call that needs none of the export's scratch)
    void fill(void *p, int v, size_t b) const { HIP_OK(hipMemsetAsync(p, v, b ? b : 1, s)); }
    void read(void *host, const void *dev, size_t b) const { HIP_OK(hipMemcpyAsync(host, dev, b, hipMemcpyDeviceToHost, s)); }
    void write(const void *dev, const void *host, size_t b) const { if (b) HIP_OK(hipMemcpyAsync(const_cast<void *>(dev), host, b, hipMemcpyHostToDevice, s)); }
    void sync() const { HIP_OK(hipStreamSynchronize(s)); }
};

// the id map of a mapped export: the caller's table, the kernels' arguments and the window's ids
struct MapJob { agx_idmap *m; agx_idmap_args M{}; agx_u32 n_wids = 0; };

// what the edge-support calls refuse: agx_unit_front's preconditions and the flag
static void support_check(const agx_unit *u) {
    if (!(u->prm.flags & AGX_FLAG_EDGE_SUPPORT)) throw Error{E_ARG, "edge support: the unit was created without AGX_FLAG_EDGE_SUPPORT (the counters are reserved with the unit's block)"};
    if (u->prm.flags & AGX_FLAG_ONE_SHOT) throw Error{E_ARG, "edge support: a one-shot unit gives the arrays the counting reads away with its only download"};
    if (!u->built || u->trimmed || u->downloaded) throw Error{E_ARG, "edge support: the unit is not built (call agx_unit_build; not after agx_unit_download, agx_unit_trim or agx_unit_release)"};
}

// The edge counters of the last build, made on the first request after it: cleared — e_cnt, ovf_cnt, the unmatched word; the per-tile totals are written for
// every tile —, counted by agx_k_edge_support on the export's stream, the totals read back and summed.  They stay valid until the next build, upload or release.
static void ensure_support(const Export &E) {
    agx_unit *u = E.u;
    const double t0 = now_ms();
    if (!u->support_valid) {
        const size_t nt = u->n_tiles;
        agx_support_kargs K; fill_sweep_args(u, K.S);
        K.ovf = u->d_ovf.p; K.n_ovf = E.n_ovf; K.n_hits = (agx_u32)u->nh; K.list_cap = u->list_cap;
        K.e_cnt = u->d_e_cnt.p; K.ovf_cnt = u->d_ovf_cnt.p; K.tile_events = u->d_sup_tot.p; K.tile_adds = u->d_sup_tot.p + nt; K.unmatched = u->d_sup_tot.p + 2 * nt;
        K.abort = u->d_words.p + W_STATUS;
        E.fill(K.e_cnt, 0, (size_t)u->pool_cap * AGX_MAXE * 4); E.fill(K.ovf_cnt, 0, (size_t)u->ovf_cap * 4); E.fill(u->d_sup_tot.p, 0, (2 * nt + 2) * 4);
        agx_launch_edge_support(&K, E.s);
        std::vector<agx_u32> tot(2 * nt + 1);
        E.read(tot.data(), u->d_sup_tot.p, tot.size() * 4); E.sync();
        HIP_OK(hipGetLastError());
        if (tot[2 * nt]) throw Error{E_DEVICE, "internal: edge support: " + std::to_string(tot[2 * nt]) + " contributions found no edge of the built graph"};
        uint64_t ev = 0, ad = 0;
        for (size_t t = 0; t < nt; t++) { ev += tot[t]; ad += tot[nt + t]; }
        u->sup_events = ev; u->sup_adds = ad; u->support_valid = true;
        u->stats.n_support_events = ev;
    }
    u->stats.ms_edge_support = now_ms() - t0;
}

// From "np pieces are cut" to the table in the caller's memory: phase 2 and the totals (a round trip), phase 3 and the download (another).  A is the export's view with its
// error word at `words`; R: the region export A is the local view of (nullptr: the whole export, whose head counts per position are cleared here); max_nodes bounds the bases;
// J: also the export's id map — flags read with the totals, runs beside phase 3, four more copies
// S (region exports only): also the support of every link, and where the caller wants the array — one kernel behind phase 3 and one more copy; without it the body queues what it queued before
// tail (region exports only): the body stops behind phase 3 and hands the tables over where they lie, on the device — no download is queued and t stays empty (agx_unit_bubbles)
using ExportTail = std::function<void(const Export &, const agx_unitig_region_args &, agx_u32 *words, agx_u32 ns, agx_u32 nb, agx_u32 nl)>;
static void export_body(const Export &E, agx_unitig_args &A, const agx_unitig_region_args *R, agx_u32 *words, agx_u32 np, agx_u32 max_nodes, agx_unitigs *t, MapJob *J, uint32_t **S = nullptr,
                        const ExportTail *tail = nullptr) {
    A.piece_cap = np;
    agx_u32 rounds = 1; while (rounds < 32 && (1ull << (rounds - 1)) < np) rounds++;      // ceil(log2 np) + 1
    E.fill(A.p_seg, 0xFF, (size_t)np * 4);
    if (!R) E.fill(A.hcnt, 0, ((size_t)A.n_pos + 1) * 4);
    E.fill(A.s_len, 0, ((size_t)np + 1) * 4); E.fill(A.s_links, 0, ((size_t)np + 1) * 4); E.fill(A.s_cov, 0, (size_t)np * 8);
    agx_launch_unitig_phase2(&A, R, rounds, E.s);
    E.fill(A.l_cur, 0, ((size_t)np + 1) * 4);          // (the region's lie over the pointer jumping's second ancestor array: behind the rank kernel)
    agx_launch_unitig_totals(&A, words + 4, E.s);
    agx_u32 h[4] = {0, 0, 0, 0}, nr = 0;
    if (J) {      // run starts and their scan, on the (segment, rank) the rank kernel left per local id; the run count comes with the totals
        agx_launch_idmap_flags(R, &J->M, E.s);
        E.read(&nr, J->M.foff + J->n_wids, 4);
    }
    E.read(h, words + 4, 16); E.sync();
    if (h[3]) throw Error{E_DEVICE, "unitigs: the unitig ranks are inconsistent (error word " + std::to_string(h[3]) + ")"};
    const agx_u32 ns = h[0], nb = h[1], nl = h[2];
    if (ns > np || nb > max_nodes || nb > A.seq_cap || nl > A.link_cap) throw Error{E_DEVICE, "unitigs: segment totals out of range"};
    A.seq_cap = nb; A.link_cap = nl;
    if (J) {
        if (nr > J->M.run_cap) throw Error{E_DEVICE, "unitigs: more runs in the id map than nodes in the region"};
        J->M.run_cap = nr;
    }
    agx_launch_unitig_phase3(&A, R, E.s);
    if (J) agx_launch_idmap_runs(R, &J->M, E.s);
    if (S && nl) {      // (the array grows by half when it must: what a regrow leaves behind stays in the arena until the unit is released)
        E.u->d_lsup.alloc(E.u->arena, (size_t)nl + nl / 2 + 64); E.u->stats.device_bytes = E.u->arena.capacity();
        agx_launch_unitig_link_support(R, E.u->d_flags.p, E.u->d_e_cnt.p, E.u->d_ovf_cnt.p, E.u->d_lsup.p, E.s);
    }
    if (tail && R) { (*tail)(E, *R, words, ns, nb, nl); return; }
    // the compact arrays (per-node arrays never leave the device) into pinned memory, then into the caller's malloc'd table
    const size_t o_hp = 0, o_hv = o_hp + 4 * (size_t)ns, o_ln = o_hv + 4 * (size_t)ns, o_lp = o_ln + 4 * (size_t)ns, o_cov = (o_lp + 4 * (size_t)ns + 7) & ~(size_t)7,
                 o_so = o_cov + 8 * (size_t)ns, o_lo = o_so + 4 * ((size_t)ns + 1), o_lt = o_lo + 4 * ((size_t)ns + 1), o_seq = o_lt + 4 * (size_t)nl,
                 o_run = (o_seq + nb + 3) & ~(size_t)3, o_sup = o_run + 16 * (size_t)nr, o_end = o_sup + (S ? 4 * (size_t)nl : 0);      // (runs: only with an id map; support: only on request)
    PBuf<char> pin; pin.alloc(o_end + 8);
    auto down = [&](size_t o, const void *src, size_t b) { if (b) E.read(pin.p + o, src, b); };
    down(o_hp, A.s_hpos, 4 * (size_t)ns); down(o_hv, A.s_hvar, 4 * (size_t)ns); down(o_ln, A.s_len, 4 * (size_t)ns); down(o_lp, A.s_last, 4 * (size_t)ns);
    down(o_cov, A.s_cov, 8 * (size_t)ns); down(o_so, A.s_off, 4 * ((size_t)ns + 1)); down(o_lo, A.l_off, 4 * ((size_t)ns + 1)); down(o_lt, A.l_to, 4 * (size_t)nl); down(o_seq, A.seq, nb);
    if (J) { down(o_run, J->M.r_first, 4 * (size_t)nr); down(o_run + 4 * (size_t)nr, J->M.r_last, 4 * (size_t)nr); down(o_run + 8 * (size_t)nr, J->M.r_seg, 4 * (size_t)nr); down(o_run + 12 * (size_t)nr, J->M.r_rank, 4 * (size_t)nr); }
    if (S && nl) down(o_sup, E.u->d_lsup.p, 4 * (size_t)nl);
    E.read(h, words, 4); E.sync();
    if (h[0]) throw Error{E_DEVICE, "unitigs: the segments are inconsistent (error word " + std::to_string(h[0]) + ")"};
    if (S && nl) {
        *S = (uint32_t *)malloc(4 * (size_t)nl);
        if (!*S) throw Error{E_ARG, "out of host memory"};
        memcpy(*S, pin.p + o_sup, 4 * (size_t)nl);
    }
    t->n_segs = ns; t->n_links = nl; t->n_bases = nb;
    t->head_pos = (uint32_t *)malloc(4 * ((size_t)ns + 1)); t->head_var = (uint32_t *)malloc(4 * ((size_t)ns + 1)); t->n_nodes = (uint32_t *)malloc(4 * ((size_t)ns + 1));
    t->last_pos = (uint32_t *)malloc(4 * ((size_t)ns + 1)); t->coverage = (uint64_t *)malloc(8 * ((size_t)ns + 1)); t->seq_off = (uint64_t *)malloc(8 * ((size_t)ns + 1));
    t->seq = (char *)malloc((size_t)nb + 1); t->link_from = (uint32_t *)malloc(4 * ((size_t)nl + 1)); t->link_to = (uint32_t *)malloc(4 * ((size_t)nl + 1));
    if (!t->head_pos || !t->head_var || !t->n_nodes || !t->last_pos || !t->coverage || !t->seq_off || !t->seq || !t->link_from || !t->link_to) throw Error{E_ARG, "out of host memory"};
    memcpy(t->head_pos, pin.p + o_hp, 4 * (size_t)ns); memcpy(t->head_var, pin.p + o_hv, 4 * (size_t)ns); memcpy(t->n_nodes, pin.p + o_ln, 4 * (size_t)ns);
    memcpy(t->last_pos, pin.p + o_lp, 4 * (size_t)ns); memcpy(t->coverage, pin.p + o_cov, 8 * (size_t)ns); memcpy(t->link_to, pin.p + o_lt, 4 * (size_t)nl); memcpy(t->seq, pin.p + o_seq, nb);
    t->seq[nb] = 0;
    const agx_u32 *so = (const agx_u32 *)(pin.p + o_so), *lo = (const agx_u32 *)(pin.p + o_lo);
    for (size_t g = 0; g <= ns; g++) t->seq_off[g] = so[g];      // (a unit's nodes are counted in 32 bits, so are its bases)
    for (size_t g = 0; g < ns; g++) {
        if (lo[g] > lo[g + 1] || lo[g + 1] > nl) throw Error{E_DEVICE, "unitigs: link offsets out of range"};
        for (agx_u32 i = lo[g]; i < lo[g + 1]; i++) t->link_from[i] = (uint32_t)g;
    }
    if (J && nr) {
        agx_idmap *m = J->m;
        m->id_first = (uint32_t *)malloc(4 * (size_t)nr); m->id_last = (uint32_t *)malloc(4 * (size_t)nr); m->seg = (uint32_t *)malloc(4 * (size_t)nr); m->rank_first = (uint32_t *)malloc(4 * (size_t)nr);
        if (!m->id_first || !m->id_last || !m->seg || !m->rank_first) throw Error{E_ARG, "out of host memory"};
        memcpy(m->id_first, pin.p + o_run, 4 * (size_t)nr); memcpy(m->id_last, pin.p + o_run + 4 * (size_t)nr, 4 * (size_t)nr);
        memcpy(m->seg, pin.p + o_run + 8 * (size_t)nr, 4 * (size_t)nr); memcpy(m->rank_first, pin.p + o_run + 12 * (size_t)nr, 4 * (size_t)nr);
        m->n_runs = nr;
        // what the kernels wrote must be a map: runs in id order, inside one block of ids, inside their segments
        for (agx_u32 r = 0; r < nr; r++) {
            const uint32_t a = m->id_first[r], b = m->id_last[r];
            if (a > b || b >= E.u->n_ids || (a < E.n_pos) != (b < E.n_pos) || (r && m->id_last[r - 1] >= a) || m->seg[r] >= ns ||
                (uint64_t)m->rank_first[r] + (b - a) >= t->n_nodes[m->seg[r]]) throw Error{E_DEVICE, "unitigs: the id map is inconsistent (run " + std::to_string(r) + ")"};
        }
    }
}

// The whole export.  Three host round trips: the piece count (the pointer jumping's rounds and arrays), the totals (segments, bases, links), the download.
int agx_unit_unitigs(agx_unit *u, agx_unitigs *t) {
    return answer(u, t, agx_unitigs_free, true, [&] {
        export_check(u, false);
        Export E(u);
        const agx_u32 n_pos = E.n_pos, cap = E.cap, n_ovf = E.n_ovf;
        if (!n_pos || !cap || !u->n_nodes) return;
        E.open(unitig_layout(cap, n_pos, n_ovf, nullptr, nullptr, nullptr));
        agx_unitig_args A{}; agx_u32 *words = nullptr;
        unitig_layout(cap, n_pos, n_ovf, u->d_ut.p, &A, &words);
        A.node_start = u->d_node_start.p; A.node_cnt = u->d_node_cnt.p; A.n_flags = u->d_flags.p; A.n_base = u->d_base.p; A.n_next = u->d_next.p;
        A.n_counts = u->d_counts.p; A.ref = u->d_ref.p; A.ovf = u->d_ovf.p; A.n_ovf = n_ovf; A.n_pos = n_pos; A.pool_cap = cap; A.piece_cap = cap; A.err = words;
        const size_t nwin = ((size_t)cap + 63) / 64;
        E.fill(words, 0, 32); E.fill(A.pos_of, 0xFF, (size_t)cap * 4); E.fill(A.indeg, 0, (size_t)cap * 4); E.fill(A.oout, 0, (size_t)cap * 4); E.fill(A.haspred, 0, cap);
        E.fill(A.ovf_hash, 0xFF, ((size_t)A.hash_mask + 1) * 8); E.fill(A.wcnt, 0, (nwin + 1) * 4);
        agx_launch_unitig_phase1(&A, E.s);
        agx_u32 h[2] = {0, 0};
        E.read(h, words, 4); E.read(h + 1, A.woff + nwin, 4); E.sync();
        if (h[0] & 1u) throw Error{E_DEVICE, "unitigs: an edge of the node table does not lead to a later position (the graph is not a DAG)"};
        if (h[0]) throw Error{E_DEVICE, "unitigs: the node table is inconsistent (error word " + std::to_string(h[0]) + ")"};
        const agx_u32 np = h[1];
        if (np > cap) throw Error{E_DEVICE, "unitigs: more pieces than node slots"};
        export_body(E, A, nullptr, words, np, u->n_nodes, t, nullptr);
    });
}

// Region export (DESIGN.md §11 "A region at a chosen coverage"): the unitigs of the sub-graph of positions [pos_lo, pos_hi) whose nodes are alive at min_coverage.  The same
// scratch buffer, a stream of its own; no launch and no memset below is sized by the unit's positions or node slots, only by the window's positions, its kept nodes and the
// overflow list (which has no position index).  Four host round trips: the kept nodes, the piece and head counts, and export_body's two (the totals, the download) — the
// whole export above comes through the same body with one trip less in front of it.
// (m: also the id map of the export, agx_unit_unitigs_mapped; nullptr: every command and copy is agx_unit_unitigs_region's; link_support: also the links' support,
// agx_unit_unitigs_support — the counters are made first if this is the first request since the build)
// (tail: export_body's — the front runs unchanged and the tables stay on the device)
static void region_export(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t, agx_idmap *m, uint32_t **link_support = nullptr, const ExportTail *tail = nullptr) {
    if (link_support) support_check(u);
    export_check(u, m != nullptr);
    window_check(u, pos_lo, pos_hi, "unitigs: region");
    Export E(u);
    const agx_u32 n_pos = E.n_pos, cap = E.cap, n_ovf = E.n_ovf, n_win = pos_hi - pos_lo;
    if (m) { m->n_pos = n_pos; m->n_ids = u->n_ids; }
    if (!n_win || !cap || !u->n_nodes) return;
    // (the buffer of the whole export: the room the upload reserved; a tiny unit: unitig_region_layout)
    E.open(std::max(unitig_layout(cap, n_pos, n_ovf, nullptr, nullptr, nullptr), unitig_region_layout(cap, n_win, std::min<size_t>(u->n_nodes, cap), n_ovf, nullptr, nullptr, nullptr)));
    if (link_support) ensure_support(E);
    agx_unitig_region_args R{}; agx_u32 *words = nullptr;
    auto bind = [&](agx_u32 kept) {
        R = agx_unitig_region_args{};
        unitig_region_layout(cap, n_win, kept, n_ovf, u->d_ut.p, &R, &words);
        agx_unitig_args &A = R.U;
        A.node_start = u->d_node_start.p; A.n_base = u->d_base.p; A.n_next = u->d_next.p; A.n_counts = u->d_counts.p; A.ref = u->d_ref.p; A.ovf = u->d_ovf.p; A.n_ovf = n_ovf;
        A.pool_cap = kept; A.piece_cap = kept; A.n_pos = (kept + 63u) / 64u; A.err = words;
        R.nk_cid = u->d_cid.p; R.node_cnt = u->d_node_cnt.p; R.pos_lo = pos_lo; R.n_win = n_win; R.min_cov = min_coverage; R.pool_cap = cap;
    };
    bind(0);
    E.fill(words, 0, 32);
    agx_launch_unitig_region_count(&R, E.s);
    agx_u32 h[3] = {0, 0, 0}, hm[2] = {0, 0};      // hm: the id map's side-id bounds
    MapJob J{m};
    agx_idmap_args &M = J.M;
    if (m) {      // the window's side ids: two bisections on the device, read with the kept nodes
        M.a_nid = u->d_a_nid.p; M.side_xpos = u->d_side_xpos.p; M.n_pos = n_pos; M.n_ids = u->n_ids; M.n_main = n_win; M.bounds = words + 1;
        agx_launch_idmap_bounds(&R, &M, E.s);
        E.read(hm, words + 1, 8);
    }
    E.read(h, words, 4); E.read(h + 1, R.offw + n_win, 4); E.sync();
    if (h[0]) throw Error{E_DEVICE, "unitigs: the node table is inconsistent (error word " + std::to_string(h[0]) + ")"};
    const agx_u32 kept = h[1];
    if (kept > u->n_nodes || kept > cap) throw Error{E_DEVICE, "unitigs: more nodes in the region than in the unit"};
    if (!kept) return;
    bind(kept);
    if (m) {
        const agx_u32 sides = u->n_ids > n_pos ? u->n_ids - n_pos : 0u;
        if (hm[0] > hm[1] || hm[1] > sides) throw Error{E_DEVICE, "unitigs: the side ids are not in position order"};
        M.side_lo = hm[0]; M.n_side = hm[1] - hm[0]; J.n_wids = n_win + M.n_side;
        idmap_layout((size_t)n_pos + sides, std::min<size_t>(std::min<size_t>(u->n_nodes, cap), (size_t)n_pos + sides), u->d_ut.p + E.map_at, &M);      // (the layout the buffer was sized by: this window's ids fit its front)
        M.run_cap = (agx_u32)std::min<size_t>(kept, J.n_wids);
    }
    agx_unitig_args &A = R.U;
    const size_t ngrp = A.n_pos;
    if (n_ovf) E.fill(A.ovf_hash, 0xFF, ((size_t)A.hash_mask + 1) * 8);
    E.fill(A.wcnt, 0, (ngrp + 1) * 4); E.fill(A.hcnt, 0, (ngrp + 1) * 4);
    agx_launch_unitig_region_phase1(&R, E.s);
    E.read(h, words, 4); E.read(h + 1, A.woff + ngrp, 4); E.read(h + 2, A.hoff + ngrp, 4); E.sync();
    if (h[0] & 1u) throw Error{E_DEVICE, "unitigs: an edge of the node table does not lead to a later position (the graph is not a DAG)"};
    if (h[0]) throw Error{E_DEVICE, "unitigs: the node table is inconsistent (error word " + std::to_string(h[0]) + ")"};
    const agx_u32 np = h[1];
    if (!np || np > kept || h[2] > np) throw Error{E_DEVICE, "unitigs: piece and head counts out of range"};
    export_body(E, A, &R, words, np, kept, t, m ? &J : nullptr, link_support, tail);
}

int agx_unit_unitigs_region(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t) {
    return answer(u, t, agx_unitigs_free, true, [&] { region_export(u, pos_lo, pos_hi, min_coverage, t, nullptr); });
}

int agx_unit_unitigs_mapped(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t, agx_idmap *m) {
    if (!u || !t || !m) return AGX_E_ARG;
    memset(t, 0, sizeof *t); memset(m, 0, sizeof *m);
    const int rc = guarded(u, [&] { region_export(u, pos_lo, pos_hi, min_coverage, t, m); });
    if (rc != AGX_OK) { agx_unitigs_free(t); agx_idmap_free(m); }
    return rc;
}

void agx_idmap_free(agx_idmap *m) {
    if (!m) return;
    free(m->id_first); free(m->id_last); free(m->seg); free(m->rank_first);
    memset(m, 0, sizeof *m);
}

int agx_unit_unitigs_support(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t, uint32_t **link_support, agx_idmap *m) {
    if (!u || !t || !link_support) return AGX_E_ARG;
    memset(t, 0, sizeof *t); *link_support = nullptr; if (m) memset(m, 0, sizeof *m);
    const int rc = guarded(u, [&] {
        region_export(u, pos_lo, pos_hi, min_coverage, t, m, link_support);
        if (!*link_support && !(*link_support = (uint32_t *)malloc(4))) throw Error{E_ARG, "out of host memory"};      // (no links: still an array, agx_unitigs_gfa_support refuses NULL)
    });
    if (rc != AGX_OK) { agx_unitigs_free(t); agx_link_support_free(*link_support); *link_support = nullptr; if (m) agx_idmap_free(m); }
    return rc;
}

void agx_link_support_free(uint32_t *link_support) { free(link_support); }

// The counters in agx_unit_graph's numbering.  The node table's edge arrays come down whole, as in that call, and are renumbered on the host; the overflow list's duplicates
// merge with their counts summed.
int agx_unit_edge_support(agx_unit *u, agx_edge_support *s) {
    return answer(u, s, agx_edge_support_free, true, [&] {
        support_check(u);
        Export E(u);
        E.open_stream();
        ensure_support(E);
        const agx_u32 n_pos = E.n_pos, nn = u->n_nodes, cap = E.cap, n_ovf = E.n_ovf;
        std::vector<agx_u32> node_start(n_pos), next((size_t)cap * AGX_MAXE), e_cnt((size_t)cap * AGX_MAXE), ovf_cnt(n_ovf); std::vector<agx_u16> node_cnt(n_pos); std::vector<agx_edge_ovf> ovf(n_ovf);
        if (n_pos) { E.read(node_start.data(), u->d_node_start.p, (size_t)n_pos * 4); E.read(node_cnt.data(), u->d_node_cnt.p, (size_t)n_pos * 2); }
        if (cap) { E.read(next.data(), u->d_next.p, next.size() * 4); E.read(e_cnt.data(), u->d_e_cnt.p, e_cnt.size() * 4); }
        if (n_ovf) { E.read(ovf.data(), u->d_ovf.p, (size_t)n_ovf * sizeof(agx_edge_ovf)); E.read(ovf_cnt.data(), u->d_ovf_cnt.p, (size_t)n_ovf * 4); }
        E.sync();
        std::vector<agx_u32> canon, slot_of;
        number_nodes(node_start, node_cnt, cap, nn, canon, slot_of, nullptr);
        std::vector<std::vector<std::pair<agx_u32, agx_u32> > > adj(nn);      // (target, count)
        for (agx_u32 c = 0; c < nn; c++) for (agx_u32 e = 0; e < AGX_MAXE; e++) {
            const size_t at = (size_t)slot_of[c] * AGX_MAXE + e;
            if (next[at] == AGX_NONE) continue;
            if (next[at] >= cap) throw Error{E_DEVICE, "node table is inconsistent (an edge outside the pool)"};
            adj[c].emplace_back(canon[next[at]], e_cnt[at]);
        }
        for (agx_u32 i = 0; i < n_ovf; i++) {
            if (ovf[i].src >= cap || ovf[i].dst >= cap || canon[ovf[i].src] == AGX_NONE) throw Error{E_DEVICE, "node table is inconsistent (an overflow edge outside the pool)"};
            adj[canon[ovf[i].src]].emplace_back(canon[ovf[i].dst], ovf_cnt[i]);
        }
        size_t ne = 0;
        for (auto &a : adj) {
            std::sort(a.begin(), a.end());
            size_t k = 0;
            for (size_t i = 0; i < a.size(); i++) { if (k && a[k - 1].first == a[i].first) a[k - 1].second += a[i].second; else a[k++] = a[i]; }
            a.resize(k); ne += k;
        }
        s->n_nodes = nn; s->n_edges = (uint32_t)ne; s->n_events = u->sup_events; s->n_contributions = u->sup_adds;
        s->edge_start = (uint32_t *)malloc(4 * ((size_t)nn + 1)); s->edge_dst = (uint32_t *)malloc(4 * (ne + 1)); s->edge_cnt = (uint32_t *)malloc(4 * (ne + 1));
        if (!s->edge_start || !s->edge_dst || !s->edge_cnt) throw Error{E_ARG, "out of host memory"};
        size_t eo = 0;
        for (agx_u32 c = 0; c < nn; c++) { s->edge_start[c] = (uint32_t)eo; for (const auto &d : adj[c]) { s->edge_dst[eo] = d.first; s->edge_cnt[eo++] = d.second; } }
        s->edge_start[nn] = (uint32_t)eo;
    });
}

void agx_edge_support_free(agx_edge_support *s) {
    if (!s) return;
    free(s->edge_start); free(s->edge_dst); free(s->edge_cnt); memset(s, 0, sizeof *s);
}

// Edge reads: the hits behind the selected edges of a window.  Per chunk of the window's tiles two host round trips — the count pass and its scan (the total
// comes back), the emit pass (the records come back) —, then one more for the whole call: the counters of the listed edges (agx_k_edge_reads_support), which are the table's
// `support` and must equal the number of hits each edge lists.  The scratch is the export's buffer; what does not fit goes through in smaller chunks.
static void edge_reads(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t max_support, agx_edge_reads *r) {
    const double t0 = now_ms();
    support_check(u);
    if (!(u->prm.flags & AGX_FLAG_KEEP_COUNTS)) throw Error{E_ARG, "edge reads: the unit was created without AGX_FLAG_KEEP_COUNTS (the scratch is the export's buffer, which only such units reserve)"};
    window_check(u, pos_lo, pos_hi, "edge reads: window");
    struct Rec { agx_u32 sp, dp, vars, hit; };
    static_assert(sizeof(Rec) == 16, "a record is four words");
    std::vector<Rec> recs;
    std::vector<agx_u32> sup;
    unsigned n_chunks = 0;
    Export E(u);
    const agx_u32 n_pos = E.n_pos, cap = E.cap, n_ovf = E.n_ovf;
    if (pos_lo < pos_hi && cap && u->n_nodes && u->n_tiles) {
        E.open();
        ensure_support(E);
        const size_t avail = u->d_ut.n;
        const agx_u32 t_lo = pos_lo / AGX_TILE, t_hi = std::min<agx_u32>((pos_hi + AGX_TILE - 1) / AGX_TILE, u->n_tiles);
        auto fixed = [](size_t tiles) { return edge_reads_layout(tiles, 0, nullptr, nullptr, nullptr) + 16; };
        size_t chunk = t_hi - t_lo;
        if (const char *env = getenv("AGX_EDGE_READS_CHUNK")) { const long long v = atoll(env); if (v > 0) chunk = std::min<size_t>((size_t)v, chunk); }
        chunk = std::min<size_t>(chunk, (0xFFFFFF00u / AGX_TILE));
        while (chunk > 1 && fixed(chunk) > avail) chunk = (chunk + 1) / 2;
        if (fixed(chunk) > avail) throw Error{E_UNSUPPORTED, "edge reads: the export's scratch of " + std::to_string(avail) + " bytes does not hold the counts of one tile"};
        // A chunk's total is a 32-bit scan.  A selection is a part of all contributions, so it cannot wrap while those number less than 2^32; a unit with more has its
        // chunks cut where the per-tile totals of the counting pass (still in d_sup_tot) say a chunk could reach 2^32.
        std::vector<agx_u32> tile_adds;
        if (u->sup_adds >= 0xFFFFFFFFull) { tile_adds.resize(u->n_tiles); E.read(tile_adds.data(), u->d_sup_tot.p + u->n_tiles, (size_t)u->n_tiles * 4); E.sync(); }
        agx_reads_kargs K{}; fill_sweep_args(u, K.S);
        agx_reads_tab &T = K.T;
        T.n_next = u->d_next.p; T.n_flags = u->d_flags.p; T.ovf = u->d_ovf.p; T.n_ovf = n_ovf; T.e_cnt = u->d_e_cnt.p; T.ovf_cnt = u->d_ovf_cnt.p;
        T.pos_lo = pos_lo; T.pos_hi = pos_hi; T.max_support = max_support;
        K.perm = u->d_perm.p; K.n_hits = (agx_u32)u->nh; K.list_cap = u->list_cap; K.abort = u->d_words.p + W_STATUS;
        auto failed = [](agx_u32 w) {
            return Error{E_DEVICE, std::string("internal: edge reads: ") + ((w & 1u) ? "a contribution found no edge of the built graph" : "the emit pass disagrees with its count") + " (error word " + std::to_string(w) + ")"};
        };
        for (agx_u32 t = t_lo; t < t_hi;) {
            size_t nt = std::min<size_t>(chunk, t_hi - t);
            if (!tile_adds.empty()) {
                uint64_t s = 0; size_t fit = 0;
                while (fit < nt && s + tile_adds[t + fit] < 0xFFFFFFFFull) s += tile_adds[t + fit++];
                nt = std::max<size_t>(fit, 1);
            }
            agx_u32 total = 0, w = 0; agx_u32 *words = nullptr; size_t n = 0;
            for (;;) {      // the count pass, again over half the tiles while the records do not fit behind the counts
                n = nt * AGX_TILE;
                edge_reads_layout(nt, 0, u->d_ut.p, &K, &words);
                K.tile_lo = t; K.n_tiles = (agx_u32)nt; K.emit = 0; K.rec_cap = 0;
                E.fill(words, 0, 32); E.fill(K.cnt + n, 0, 4);
                agx_launch_edge_reads(&K, E.s);
                agx_launch_exclusive_scan(K.cnt, K.off, (agx_u32)n, K.scan_tmp, E.s);
                E.read(&total, K.off + n, 4); E.read(&w, words, 4); E.sync();
                HIP_OK(hipGetLastError());
                if (w) throw failed(w);
                if ((size_t)total <= (avail - fixed(nt)) / 16) break;
                if (nt == 1) throw Error{E_UNSUPPORTED, "edge reads: the " + std::to_string(total) + " records of tile " + std::to_string(t) + " do not fit the export's scratch of " + std::to_string(avail) + " bytes"};
                nt = (nt + 1) / 2; chunk = nt;
            }
            n_chunks++;
            if (total) {
                if ((uint64_t)recs.size() + total >= 0xFFFFFFFFull) throw Error{E_UNSUPPORTED, "edge reads: 2^32 listed hits or more"};
                K.emit = 1; K.rec_cap = total;
                agx_launch_edge_reads(&K, E.s);
                const size_t at = recs.size();
                recs.resize(at + total);
                E.read(recs.data() + at, K.recs, (size_t)total * 16); E.read(&w, words, 4); E.sync();
                HIP_OK(hipGetLastError());
                if (w) throw failed(w);
            }
            t += (agx_u32)nt;
        }
        // canonical order: edges by (src_pos, src_var, dst_pos, dst_var).  The host only groups, stably: that an edge's hits ascend is the device's doing (a lane walks its
        // list in order, the list is ranked by hit number) and is checked below, not made here
        auto key = [](const Rec &a) { return std::make_tuple(a.sp, a.vars & 0xFFFFu, a.dp, a.vars >> 16); };
        if (!std::is_sorted(recs.begin(), recs.end(), [&](const Rec &a, const Rec &b) { return key(a) < key(b); }))
            std::stable_sort(recs.begin(), recs.end(), [&](const Rec &a, const Rec &b) { return key(a) < key(b); });
        // the counters of the listed edges, in pieces the scratch holds: three words in and one out per edge
        std::vector<agx_u32> e_sp, e_dp, e_vars;
        for (size_t i = 0; i < recs.size(); i++)
            if (!i || recs[i].sp != recs[i - 1].sp || recs[i].dp != recs[i - 1].dp || recs[i].vars != recs[i - 1].vars) { e_sp.push_back(recs[i].sp); e_dp.push_back(recs[i].dp); e_vars.push_back(recs[i].vars); }
        const size_t ne = e_sp.size(), piece = std::max<size_t>((avail - 2048) / 16, 1);
        sup.resize(ne);
        for (size_t at = 0; at < ne; at += piece) {
            const size_t m = std::min(piece, ne - at);
            Carve take{u->d_ut.p};
            agx_reads_sup_args S{}; S.T = T; S.node_start = u->d_node_start.p; S.node_cnt = u->d_node_cnt.p; S.n_pos = n_pos; S.pool_cap = cap; S.n = (agx_u32)m;
            take(S.sp, m); take(S.dp, m); take(S.vars, m); take(S.sup, m);
            E.write(S.sp, e_sp.data() + at, m * 4); E.write(S.dp, e_dp.data() + at, m * 4); E.write(S.vars, e_vars.data() + at, m * 4);
            agx_launch_edge_reads_support(&S, E.s);
            E.read(sup.data() + at, S.sup, m * 4); E.sync();
            HIP_OK(hipGetLastError());
        }
    }
    // the caller's table
    const size_t nh = recs.size(), ne = sup.size();
    host_array(r->src_pos, ne); host_array(r->src_var, ne); host_array(r->dst_pos, ne); host_array(r->dst_var, ne); host_array(r->support, ne); host_array(r->hit_off, ne + 1); host_array(r->hit, nh);
    size_t e = 0;
    for (size_t i = 0; i < nh; i++) {
        const bool first = !i || recs[i].sp != recs[i - 1].sp || recs[i].dp != recs[i - 1].dp || recs[i].vars != recs[i - 1].vars;
        if (first) { r->src_pos[e] = recs[i].sp; r->src_var[e] = recs[i].vars & 0xFFFFu; r->dst_pos[e] = recs[i].dp; r->dst_var[e] = recs[i].vars >> 16; r->support[e] = sup[e]; r->hit_off[e] = i; e++; }
        else if (recs[i].hit <= recs[i - 1].hit)
            throw Error{E_DEVICE, "internal: edge reads: the hits behind an edge do not ascend (hit " + std::to_string(recs[i].hit) + " behind hit " + std::to_string(recs[i - 1].hit) + ": listed twice, or emitted out of order)"};
        r->hit[i] = recs[i].hit;
    }
    r->hit_off[ne] = nh; r->n_edges = (uint32_t)ne; r->n_hits = nh;
    for (size_t i = 0; i < ne; i++)
        if (r->hit_off[i + 1] - r->hit_off[i] != r->support[i])
            throw Error{E_DEVICE, "internal: edge reads: the edge (" + std::to_string(r->src_pos[i]) + ", " + std::to_string(r->src_var[i]) + ") -> (" + std::to_string(r->dst_pos[i]) + ", " + std::to_string(r->dst_var[i]) +
                                  ") lists " + std::to_string(r->hit_off[i + 1] - r->hit_off[i]) + " hits, its counter holds " + std::to_string(r->support[i])};
    u->stats.ms_edge_reads = now_ms() - t0;
    if (g_trace) fprintf(stderr, "[agx trace] unit %p edge reads [%u, %u) <= %u: %u chunks, %zu records of 16 bytes, %zu edges\n", (void *)u, pos_lo, pos_hi, max_support, n_chunks, nh, ne);
    trace(u, "edge_reads", t0, u->V.n_pos);
}

int agx_unit_edge_reads(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t max_support, agx_edge_reads *r) {
    return answer(u, r, agx_edge_reads_free, true, [&] { edge_reads(u, pos_lo, pos_hi, max_support, r); });
}

void agx_edge_reads_free(agx_edge_reads *r) {
    if (!r) return;
    free(r->src_pos); free(r->src_var); free(r->dst_pos); free(r->dst_var); free(r->support); free(r->hit_off); free(r->hit);
    memset(r, 0, sizeof *r);
}

int agx_unit_walk_paths(agx_unit *u, agx_walk_paths *w) {
    return answer(u, w, agx_walk_paths_free, true, [&] {
        if (!(u->prm.flags & AGX_FLAG_KEEP_PATHS)) throw Error{E_ARG, "walk paths: the unit was created without AGX_FLAG_KEEP_PATHS"};
        if (!u->out.paths_ready) throw Error{E_ARG, "walk paths: nothing kept (call agx_unit_finish; not after another upload or agx_unit_release)"};
        const WalkPaths &P = u->out.paths;
        const size_t nr = P.rec_len.size(), ns = P.id_first.size();
        if (nr >= 0xFFFFFFFFull) throw Error{E_OVERFLOW, "walk paths: more than 2^32 records"};
        w->rec_len = (uint64_t *)malloc(8 * (nr + 1)); w->st_off = (uint64_t *)malloc(8 * (nr + 1)); w->id_first = (uint32_t *)malloc(4 * (ns + 1)); w->id_last = (uint32_t *)malloc(4 * (ns + 1));
        w->base_off = (uint64_t *)malloc(8 * (ns + 1)); w->joined = (uint8_t *)malloc(ns + 1);
        if (!w->rec_len || !w->st_off || !w->id_first || !w->id_last || !w->base_off || !w->joined) throw Error{E_ARG, "out of host memory"};
        w->n_recs = (uint32_t)nr; w->n_stretches = ns;
        if (nr) memcpy(w->rec_len, P.rec_len.data(), 8 * nr);
        w->st_off[0] = 0; if (nr) memcpy(w->st_off + 1, P.st_end.data(), 8 * nr);
        if (ns) { memcpy(w->id_first, P.id_first.data(), 4 * ns); memcpy(w->id_last, P.id_last.data(), 4 * ns); memcpy(w->base_off, P.base_off.data(), 8 * ns); memcpy(w->joined, P.joined.data(), ns); }
    });
}

void agx_walk_paths_free(agx_walk_paths *w) {
    if (!w) return;
    free(w->rec_len); free(w->st_off); free(w->id_first); free(w->id_last); free(w->base_off); free(w->joined);
    memset(w, 0, sizeof *w);
}

// A caller's stretch table (agx_walk_paths), checked against the unit and flattened into the form the device reads (agx_evidence_tab): what agx_unit_walk_evidence and
// agx_unit_walk_span both ask of a table, with the asking call's name in front of the reason.  tracks: rec_lo <= rec_hi <= n_recs is asked too.
struct FlatTable {
    size_t nr = 0, ns = 0; uint64_t total = 0;      // records, stretches, graph bases
    std::vector<agx_u32> st_first, st_base, st_rec, st_pre; std::vector<agx_u8> st_join; std::vector<uint64_t> rec_bases;
    // the device's view: the unit's arrays, and the five stretch arrays uploaded to where the call's layout carved them (e_cnt, ovf_cnt: the edge counters, or null)
    void bind(const Export &E, agx_evidence_tab &T, const agx_u32 *e_cnt, const agx_u32 *ovf_cnt) const {
        const agx_unit *u = E.u;
        T.n_st = (agx_u32)ns; T.n_flat = (agx_u32)total;
        T.a_nid = u->d_a_nid.p; T.n_ids = u->n_ids; T.pool_cap = E.cap; T.n_counts = u->d_counts.p; T.n_next = u->d_next.p; T.n_flags = u->d_flags.p; T.ovf = u->d_ovf.p; T.n_ovf = E.n_ovf;
        T.e_cnt = e_cnt; T.ovf_cnt = ovf_cnt;
        E.write(T.st_first, st_first.data(), ns * 4); E.write(T.st_base, st_base.data(), ns * 4); E.write(T.st_rec, st_rec.data(), ns * 4); E.write(T.st_pre, st_pre.data(), (ns + 1) * 4); E.write(T.st_join, st_join.data(), ns + 1);
    }
};
static FlatTable check_walk_table(const agx_unit *u, const agx_walk_paths &w, bool tracks, uint32_t rec_lo, uint32_t rec_hi, const std::string &who) {
    const size_t nr = w.n_recs; const uint64_t ns64 = w.n_stretches;
    auto bad = [&](const std::string &why) { return Error{E_ARG, who + ": " + why}; };
    if (nr && (!w.rec_len || !w.st_off)) throw bad("the stretch table has records but no rec_len / st_off");
    if (ns64 && (!w.id_first || !w.id_last || !w.base_off || !w.joined || !nr)) throw bad("the stretch table has stretches but no arrays or no records");
    if (nr && (w.st_off[0] != 0 || w.st_off[nr] != ns64)) throw bad("st_off does not run from 0 to n_stretches");
    if (tracks && (rec_lo > rec_hi || rec_hi > nr)) throw bad("track records [" + std::to_string(rec_lo) + ", " + std::to_string(rec_hi) + ") are not within the table's " + std::to_string(nr));
    if (ns64 >= 0xFFFFFFFFull) throw Error{E_UNSUPPORTED, who + ": 2^32 stretches or more"};
    const size_t ns = (size_t)ns64;
    FlatTable F; F.nr = nr; F.ns = ns;
    F.st_first.resize(ns); F.st_base.resize(ns); F.st_rec.resize(ns); F.st_pre.resize(ns + 1); F.st_join.assign(ns + 1, 0); F.rec_bases.assign(nr, 0);
    uint64_t &total = F.total;
    for (size_t r = 0; r < nr; r++) if (w.st_off[r] > w.st_off[r + 1] || w.st_off[r + 1] > ns64) throw bad("st_off is not monotone at record " + std::to_string(r));
    for (size_t r = 0; r < nr; r++) {
        if (w.st_off[r] < w.st_off[r + 1] && w.rec_len[r] > 0xFFFFFFFFull) throw Error{E_UNSUPPORTED, who + ": record " + std::to_string(r) + " has 2^32 bases or more"};
        uint64_t end = 0;
        for (size_t i = (size_t)w.st_off[r]; i < (size_t)w.st_off[r + 1]; i++) {
            const std::string at = "stretch " + std::to_string(i) + " of record " + std::to_string(r);
            if (w.id_last[i] < w.id_first[i]) throw bad(at + ": id_last < id_first");
            if (w.id_last[i] >= u->n_ids) throw bad(at + ": id_last is not a walk id of the unit (" + std::to_string(u->n_ids) + " ids)");
            const uint64_t len = (uint64_t)w.id_last[i] - w.id_first[i] + 1;
            if (w.base_off[i] > w.rec_len[r] || len > w.rec_len[r] - w.base_off[i]) throw bad(at + " does not lie inside its record");
            const bool first = i == (size_t)w.st_off[r];
            if (!first && w.base_off[i] < end) throw bad(at + " overlaps or lies in front of the stretch before it");
            if (w.joined[i] > 1) throw bad(at + ": joined is neither 0 nor 1");
            if (w.joined[i] && (first || w.base_off[i] != end)) throw bad(at + ": joined, but not directly behind the previous stretch of the record");
            F.st_first[i] = w.id_first[i]; F.st_base[i] = (agx_u32)w.base_off[i]; F.st_rec[i] = (agx_u32)r; F.st_pre[i] = (agx_u32)total; F.st_join[i] = w.joined[i];
            end = w.base_off[i] + len; total += len; F.rec_bases[r] += len;
            if (total >= 0xFFFFFFFFull) throw Error{E_UNSUPPORTED, who + ": 2^32 graph bases or more"};
        }
    }
    F.st_pre[ns] = (agx_u32)total;
    return F;
}

// The intervals of one chunk of flat bases (rec, first, last, and two minima; `cnt` of them, in order) behind those of the chunks before it: an interval cut by the chunk's
// border — the same record, the next base offset — is one interval
static void merge_chunk_intervals(std::vector<agx_u32> (&iv)[5], const std::vector<agx_u32> (&got)[5], agx_u32 cnt, size_t nr, uint64_t lo, const std::string &who) {
    for (agx_u32 i = 0; i < cnt; i++) {
        if (got[0][i] >= nr || got[1][i] > got[2][i]) throw Error{E_DEVICE, who + ": the intervals are inconsistent (chunk at base " + std::to_string(lo) + ", interval " + std::to_string(i) + ")"};
        if (i == 0 && !iv[0].empty() && iv[0].back() == got[0][0] && (uint64_t)iv[2].back() + 1 == got[1][0]) {
            iv[2].back() = got[2][0]; iv[3].back() = std::min(iv[3].back(), got[3][0]); iv[4].back() = std::min(iv[4].back(), got[4][0]);
            continue;
        }
        for (int k = 0; k < 5; k++) iv[k].push_back(got[k][i]);
    }
}

// The caller's struct as the body under the records fills it: agx_walk_evidence and agx_walk_span hold the same arrays under the names of what they hold
struct RecordsAnswer {
    uint32_t *n_recs, *n_intervals; uint64_t *n_graph_bases, *n_steps, *n_odd_steps;      // n_odd_steps: the device's second word (the steps without an edge / not forward)
    uint64_t **rec_graph_bases, **rec_steps, **rec_sum; uint32_t **rec_min, **rec_min_at, **rec_step_min, **rec_step_min_at;
    uint32_t **iv[5];      // rec, first, last, the value's minimum, the step's minimum
    uint32_t *rec_lo, *rec_hi; uint64_t *n_track, **track_off; uint32_t **track[3];      // the tracks: three values per graph base
};
// One call under the records: how it says things, and the steps that are its own
struct RecordsCall {
    const char *who, *chunk_env;      // chunk_env: the environment's override of the chunk of flat bases
    const char *internal, *numbers;   // in front of `who` when the device's answer is inconsistent; which numbers its error word is about
    const agx_u32 *e_cnt, *ovf_cnt;   // the edge counters the gather reads, or null
    const agx_u32 *const *track_src;  // [3] where a chunk's track values lie on the device (known once `lay` has run)
    double t0, *ms;                   // when the call began and where its time goes (agx_stats): taken while the export's stream still exists, as it always was
    std::function<void(const Export &)> opened;                       // (may be empty) behind the buffer and the stream, before anything else is queued
    std::function<size_t(size_t, char *, agx_u32 **)> lay;            // the call's layout with chunks of so many bases: its size; with a base, carved there, the call's arguments filled in
    std::function<std::string(size_t)> too_large;                      // what to say when chunks of 64 bases do not fit so many bytes
    std::function<void(const Export &)> whole;                         // (may be empty) queued once, behind the uploads and the fills
    std::function<void(const Export &, agx_u32)> gather;              // per chunk (V.lo, V.n set): everything up to the interval-start flags and their scan
};

// What agx_unit_walk_evidence and agx_unit_walk_span share: the caller's per-record tables and tracks, the chunk size, the flattened table uploaded
// into the export's scratch, then the flat graph bases in chunks on the export's own stream — the call's gather (a round trip: the interval count), the intervals with
// the tracks' piece (a round trip), merged behind those of the chunks before — and at the end the per-record sums and minima and the error words (a round trip).
static void records_body(agx_unit *u, const agx_walk_paths &w, const FlatTable &F, bool tracks, uint32_t rec_lo, uint32_t rec_hi, const RecordsAnswer &O, agx_evidence_args &V, const RecordsCall &C) {
    const size_t nr = F.nr; const uint64_t total = F.total;
    const std::string who = C.who, inconsistent = std::string(C.internal) + C.who;
    // the caller's tables (the per-record ones are always produced)
    *O.n_recs = (uint32_t)nr; *O.n_graph_bases = total;
    host_array(*O.rec_graph_bases, nr); host_array(*O.rec_steps, nr); host_array(*O.rec_sum, nr); host_array(*O.rec_min, nr); host_array(*O.rec_min_at, nr); host_array(*O.rec_step_min, nr); host_array(*O.rec_step_min_at, nr);
    for (size_t r = 0; r < nr; r++) { (*O.rec_graph_bases)[r] = F.rec_bases[r]; (*O.rec_min)[r] = (*O.rec_step_min)[r] = AGX_NONE; }
    size_t s_lo = 0, s_hi = 0; uint64_t t_lo = 0, t_hi = 0;      // the tracks' stretches and flat bases
    if (tracks) {
        s_lo = nr ? (size_t)w.st_off[rec_lo] : 0; s_hi = nr ? (size_t)w.st_off[rec_hi] : 0; t_lo = F.st_pre[s_lo]; t_hi = F.st_pre[s_hi];
        *O.rec_lo = rec_lo; *O.rec_hi = rec_hi; *O.n_track = t_hi - t_lo;
        host_array(*O.track_off, s_hi - s_lo + 1);
        for (int k = 0; k < 3; k++) host_array(*O.track[k], (size_t)*O.n_track);
        for (size_t i = s_lo; i <= s_hi; i++) (*O.track_off)[i - s_lo] = F.st_pre[i] - t_lo;
    }
    Export E(u);
    E.open();
    if (C.opened) C.opened(E);
    std::vector<agx_u32> iv[5];      // rec, first, last, and the two minima
    if (total) {
        const size_t avail = u->d_ut.n;
        if (C.lay(64, nullptr, nullptr) > avail) throw Error{E_UNSUPPORTED, C.too_large(avail)};
        size_t chunk = std::min<size_t>(((size_t)total + 63) & ~(size_t)63, (size_t)1 << 30);
        if (const char *env = getenv(C.chunk_env)) { const long long v = atoll(env); if (v > 0) chunk = std::min<size_t>(((size_t)v + 63) & ~(size_t)63, (size_t)1 << 30); }
        while (chunk > 64 && C.lay(chunk, nullptr, nullptr) > avail) chunk = ((chunk / 2) + 63) & ~(size_t)63;
        agx_u32 *words = nullptr;
        C.lay(chunk, u->d_ut.p, &words);
        V.n_recs = (agx_u32)nr;
        F.bind(E, V.T, C.e_cnt, C.ovf_cnt);
        E.fill(words, 0, 32); E.fill(V.r_steps, 0, nr * 8); E.fill(V.r_dsum, 0, nr * 8); E.fill(V.r_dmin, 0xFF, nr * 8); E.fill(V.r_smin, 0xFF, nr * 8);
        if (C.whole) C.whole(E);
        std::vector<agx_u32> got[5];
        for (uint64_t lo = 0; lo < total; lo += chunk) {
            const agx_u32 n = (agx_u32)std::min<uint64_t>(chunk, total - lo);
            V.lo = (agx_u32)lo; V.n = n; V.iv_cap = 0;
            C.gather(E, n);
            agx_u32 cnt = 0;
            E.read(&cnt, V.foff + n, 4); E.sync();
            if (cnt > n) throw Error{E_DEVICE, inconsistent + ": more intervals than bases"};
            if (cnt) {
                V.iv_cap = cnt;
                E.fill(V.iv_dmin, 0xFF, (size_t)cnt * 4); E.fill(V.iv_smin, 0xFF, (size_t)cnt * 4);
                agx_launch_evidence_runs(&V, E.s);
                agx_u32 *src[5] = {V.iv_rec, V.iv_first, V.iv_last, V.iv_dmin, V.iv_smin};
                for (int k = 0; k < 5; k++) { got[k].resize(cnt); E.read(got[k].data(), src[k], (size_t)cnt * 4); }
            }
            if (tracks) {      // the piece of the tracks that lies in this chunk
                const uint64_t a = std::max<uint64_t>(lo, t_lo), b = std::min<uint64_t>(lo + n, t_hi);
                if (a < b) for (int k = 0; k < 3; k++) E.read(*O.track[k] + (a - t_lo), C.track_src[k] + (a - lo), (size_t)(b - a) * 4);
            }
            E.sync();
            merge_chunk_intervals(iv, got, cnt, nr, lo, who);
        }
        std::vector<unsigned long long> rs(nr), rd(nr), rmin(nr), smin(nr); agx_u32 wd[2] = {0, 0};
        if (nr) { E.read(rs.data(), V.r_steps, nr * 8); E.read(rd.data(), V.r_dsum, nr * 8); E.read(rmin.data(), V.r_dmin, nr * 8); E.read(smin.data(), V.r_smin, nr * 8); }
        E.read(wd, words, 8); E.sync();
        HIP_OK(hipGetLastError());
        if (wd[0]) throw Error{E_DEVICE, inconsistent + ": the " + C.numbers + " numbers are inconsistent (error word " + std::to_string(wd[0]) + ")"};
        *O.n_odd_steps = wd[1];
        for (size_t r = 0; r < nr; r++) {
            (*O.rec_steps)[r] = rs[r]; (*O.rec_sum)[r] = rd[r]; *O.n_steps += rs[r];
            if (rmin[r] != ~0ull) { (*O.rec_min)[r] = (uint32_t)(rmin[r] >> 32); (*O.rec_min_at)[r] = (uint32_t)rmin[r]; }
            if (smin[r] != ~0ull) { (*O.rec_step_min)[r] = (uint32_t)(smin[r] >> 32); (*O.rec_step_min_at)[r] = (uint32_t)smin[r]; }
        }
    }
    const size_t ni = iv[0].size();
    *O.n_intervals = (uint32_t)ni;
    for (int k = 0; k < 5; k++) { host_array(*O.iv[k], ni); if (ni) memcpy(*O.iv[k], iv[k].data(), ni * 4); }
    *C.ms = now_ms() - C.t0;
}

// Evidence under the walk's records: depth and edge support per graph base, gathered by agx_evidence.hip.  Its own: the refusals, the edge counters made
// on the first request, and one gather launch per chunk.
static void walk_evidence(agx_unit *u, const agx_walk_paths &w, uint32_t min_depth, uint32_t min_support, bool tracks, uint32_t rec_lo, uint32_t rec_hi, agx_walk_evidence *e) {
    const double t0 = now_ms();
    export_check(u, false, "walk evidence", "the depth is the kept per-node coverage", "is asked");
    const bool counted = (u->prm.flags & AGX_FLAG_EDGE_SUPPORT) != 0;
    if (min_support && !counted) throw Error{E_ARG, "walk evidence: min_support needs the edge counters (the unit was created without AGX_FLAG_EDGE_SUPPORT)"};
    // the table, before anything is uploaded
    const FlatTable F = check_walk_table(u, w, tracks, rec_lo, rec_hi, "walk evidence");
    if (counted) support_check(u);
    const size_t nr = F.nr, ns = F.ns;
    agx_evidence_args A{}; const agx_u32 *track_src[3] = {nullptr, nullptr, nullptr};
    const RecordsAnswer O{&e->n_recs, &e->n_intervals, &e->n_graph_bases, &e->n_steps, &e->n_steps_without_edge,
                          &e->rec_graph_bases, &e->rec_steps, &e->rec_depth_sum, &e->rec_depth_min, &e->rec_depth_min_at, &e->rec_step_min, &e->rec_step_min_at,
                          {&e->iv_rec, &e->iv_first, &e->iv_last, &e->iv_depth_min, &e->iv_step_min}, &e->rec_lo, &e->rec_hi, &e->n_track, &e->track_off, {&e->depth, &e->votes, &e->step}};
    RecordsCall C{"walk evidence", "AGX_EVIDENCE_CHUNK", "", "interval", counted ? u->d_e_cnt.p : nullptr, counted ? u->d_ovf_cnt.p : nullptr, track_src, t0, &u->stats.ms_walk_evidence, {}, {}, {}, {}, {}};
    C.opened = [&](const Export &E) { if (counted) ensure_support(E); };
    C.too_large = [&](size_t avail) {
        return "walk evidence: the stretch table (" + std::to_string(ns) + " stretches, " + std::to_string(nr) + " records) does not fit the export's scratch of " + std::to_string(avail) + " bytes";
    };
    C.lay = [&](size_t chunk, char *base, agx_u32 **words) {
        const size_t bytes = evidence_layout(ns, nr, chunk, tracks, base, base ? &A : nullptr, words);
        A.min_depth = min_depth; A.min_support = min_support;
        track_src[0] = A.c_depth; track_src[1] = A.c_votes; track_src[2] = A.c_step;
        return bytes;
    };
    C.gather = [&](const Export &E, agx_u32) { agx_launch_evidence_gather(&A, E.s); };
    records_body(u, w, F, tracks, rec_lo, rec_hi, O, A, C);
}

int agx_unit_walk_evidence(agx_unit *u, const agx_walk_paths *w, uint32_t min_depth, uint32_t min_support, uint32_t want_tracks, uint32_t rec_lo, uint32_t rec_hi, agx_walk_evidence *e) {
    return answer(u, e, agx_walk_evidence_free, w != nullptr, [&] { walk_evidence(u, *w, min_depth, min_support, want_tracks != 0, rec_lo, rec_hi, e); });
}

void agx_walk_evidence_free(agx_walk_evidence *e) {
    if (!e) return;
    free(e->rec_graph_bases); free(e->rec_steps); free(e->rec_depth_sum); free(e->rec_depth_min); free(e->rec_depth_min_at); free(e->rec_step_min); free(e->rec_step_min_at);
    free(e->iv_rec); free(e->iv_first); free(e->iv_last); free(e->iv_depth_min); free(e->iv_step_min);
    free(e->track_off); free(e->depth); free(e->votes); free(e->step);
    memset(e, 0, sizeof *e);
}

// Pair span.  What both calls refuse: the export's conditions, for the scratch, and the edge counting's but its flag — the pass reads the arrays the
// counting reads (the derived hit records and the runs), so it may run wherever ensure_support may.
static void span_check(const agx_unit *u, const std::string &who) {
    if (!(u->prm.flags & AGX_FLAG_KEEP_COUNTS)) throw Error{E_ARG, who + ": the unit was created without AGX_FLAG_KEEP_COUNTS (the scratch is the export's buffer, which only such units reserve)"};
    if (u->prm.flags & AGX_FLAG_ONE_SHOT) throw Error{E_ARG, who + ": a one-shot unit gives the arrays the pass reads away with its only download"};
    if (!u->built || u->trimmed || u->downloaded) throw Error{E_ARG, who + ": the unit is not built (call agx_unit_build; not after agx_unit_download, agx_unit_trim or agx_unit_release)"};
}

// span and cross of positions [lo, hi) in sub-windows of `sub` positions: per sub-window place(x) says where its start / end lie (S.start, S.end: n + 1 entries each,
// zeroed here), the kernels leave span / cross there, and done(x, n) may queue reads behind them; one host round trip each.  [lo, lo): one pass for the counts alone.
struct SpanCounts { uint64_t kept = 0, fragments = 0, outside = 0; unsigned passes = 0; };
static SpanCounts span_passes(const Export &E, agx_span_args &S, agx_u32 lo, agx_u32 hi, size_t sub, const std::string &who, const std::function<void(agx_u32)> &place,
                              const std::function<void(agx_u32, agx_u32)> &done) {
    const agx_unit *u = E.u;
    S.dhit = u->d_dhit.p; S.runs = u->d_runs.p; S.n_hits = (agx_u32)u->nh; S.n_runs = (agx_u32)u->n_runs; S.n_pos = E.n_pos; S.win_lo = lo; S.win_hi = hi;
    SpanCounts C;
    std::vector<agx_u32> part((size_t)3 * S.n_part);
    for (agx_u32 x = lo; !C.passes || x < hi;) {
        const agx_u32 n = (agx_u32)std::min<size_t>(sub, hi - x);
        S.lo = x; S.n = n;
        place(x);
        E.fill(S.start, 0, ((size_t)n + 1) * 4); E.fill(S.end, 0, ((size_t)n + 1) * 4); E.fill(S.part, 0, part.size() * 4);
        agx_launch_pair_span(&S, E.s);
        E.read(part.data(), S.part, part.size() * 4);
        done(x, n);
        E.sync();
        HIP_OK(hipGetLastError());
        uint64_t f = 0, k = 0, o = 0;
        for (size_t i = 0; i < S.n_part; i++) { f += part[3 * i]; k += part[3 * i + 1]; o += part[3 * i + 2]; }
        if (C.passes && (f != C.fragments || k != C.kept || o != C.outside)) throw Error{E_DEVICE, "internal: " + who + ": two passes over the hits disagree on their counts"};
        C.fragments = f; C.kept = k; C.outside = o; C.passes++;
        x += n;
        if (!n) break;
    }
    return C;
}

// the sub-window a call works in: the whole window, AGX_SPAN_CHUNK's, or as many positions as `bytes_of` says fit the scratch (0: not even one)
static size_t span_sub_window(size_t n, size_t avail, const std::function<size_t(size_t)> &bytes_of) {
    size_t sub = std::max<size_t>(n, 1);
    if (const char *env = getenv("AGX_SPAN_CHUNK")) { const long long v = atoll(env); if (v > 0) sub = std::min<size_t>((size_t)v, sub); }
    while (sub > 1 && bytes_of(sub) > avail) sub = (sub + 1) / 2;
    return bytes_of(sub) > avail ? 0 : sub;
}

static void pair_span(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, agx_pair_span *s) {
    const double t0 = now_ms();
    span_check(u, "pair span");
    window_check(u, pos_lo, pos_hi, "pair span: window");
    const size_t n = pos_hi - pos_lo;
    s->pos_lo = pos_lo; s->pos_hi = pos_hi;
    host_array(s->span, n); host_array(s->cross, n);
    Export E(u);
    E.open();
    const size_t avail = u->d_ut.n, parts = agx_span_partials((agx_u32)u->nh);
    const size_t sub = span_sub_window(n, avail, [&](size_t m) { return span_layout(m, parts, nullptr, nullptr); });
    if (!sub) throw Error{E_UNSUPPORTED, "pair span: the export's scratch of " + std::to_string(avail) + " bytes does not hold one position's counts beside the partial sums of " + std::to_string(u->nh) + " hits"};
    agx_span_args S{};
    span_layout(sub, parts, u->d_ut.p, &S);
    const SpanCounts C = span_passes(E, S, pos_lo, pos_hi, sub, "pair span", [](agx_u32) {}, [&](agx_u32 x, agx_u32 m) {
        if (m) { E.read(s->span + (x - pos_lo), S.start, (size_t)m * 4); E.read(s->cross + (x - pos_lo), S.end, (size_t)m * 4); }
    });
    s->n_kept = C.kept; s->n_fragments = C.fragments; s->n_outside = C.outside;
    u->stats.ms_pair_span = now_ms() - t0;
    if (g_trace) fprintf(stderr, "[agx trace] unit %p pair span [%u, %u): %u sub-windows of %zu positions, %llu kept hits, %llu fragments\n", (void *)u, pos_lo, pos_hi, C.passes, sub,
                         (unsigned long long)C.kept, (unsigned long long)C.fragments);
    trace(u, "pair_span", t0, n);
}

int agx_unit_pair_span(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, agx_pair_span *s) {
    return answer(u, s, agx_pair_span_free, true, [&] { pair_span(u, pos_lo, pos_hi, s); });
}

void agx_pair_span_free(agx_pair_span *s) {
    if (!s) return;
    free(s->span); free(s->cross);
    memset(s, 0, sizeof *s);
}

// Pair span under the walk's records: the table is checked and flattened as for the evidence and goes through the same body.  Its own: span and cross of the whole unit,
// made in the scratch before the first chunk (sub-windows where need be), and per chunk the gather (a round trip: the jump count), where there are jumps their list (a
// round trip: the host sorts and merges it), the count over the hits and the scatter, then the flags.
static void walk_span(agx_unit *u, const agx_walk_paths &w, uint32_t min_span, bool tracks, uint32_t rec_lo, uint32_t rec_hi, agx_walk_span *e) {
    const double t0 = now_ms();
    span_check(u, "walk span");
    const FlatTable F = check_walk_table(u, w, tracks, rec_lo, rec_hi, "walk span");
    const size_t nr = F.nr, ns = F.ns; const agx_u32 n_pos = (agx_u32)u->V.n_pos;
    const size_t parts = agx_span_partials((agx_u32)u->nh);
    unsigned n_chunks = 0, n_passes = 0; uint64_t n_entries = 0;
    agx_walk_span_args A{}; agx_span_args S{}; agx_evidence_args &V = A.E; agx_u32 *words = nullptr; size_t sub = 0;
    const agx_u32 *track_src[3] = {nullptr, nullptr, nullptr};
    std::vector<agx_u32> jt[3];
    SpanJumps J;
    const RecordsAnswer O{&e->n_recs, &e->n_intervals, &e->n_graph_bases, &e->n_steps, &e->n_steps_not_forward,
                          &e->rec_graph_bases, &e->rec_steps, &e->rec_span_sum, &e->rec_span_min, &e->rec_span_min_at, &e->rec_step_min, &e->rec_step_min_at,
                          {&e->iv_rec, &e->iv_first, &e->iv_last, &e->iv_span_min, &e->iv_step_min}, &e->rec_lo, &e->rec_hi, &e->n_track, &e->track_off, {&e->pos, &e->span, &e->step}};
    RecordsCall C{"walk span", "AGX_SPAN_BASE_CHUNK", "internal: ", "interval or jump", nullptr, nullptr, track_src, t0, &u->stats.ms_walk_span, {}, {}, {}, {}, {}};
    C.too_large = [&](size_t avail) {
        return "walk span: the unit's span and cross (" + std::to_string(n_pos) + " positions) and the stretch table (" + std::to_string(ns) + " stretches, " + std::to_string(nr) +
               " records) do not fit the export's scratch of " + std::to_string(avail) + " bytes";
    };
    C.lay = [&](size_t chunk, char *base, agx_u32 **w) {
        if (!base) return walk_span_layout(ns, nr, n_pos, 1, chunk, parts, nullptr, nullptr, nullptr, nullptr);
        sub = span_sub_window(n_pos, u->d_ut.n, [&](size_t m) { return walk_span_layout(ns, nr, n_pos, m, 64, parts, nullptr, nullptr, nullptr, nullptr); });
        const size_t bytes = walk_span_layout(ns, nr, n_pos, sub, chunk, parts, base, &A, &S, &words);
        *w = words;
        V.min_depth = min_span; V.min_support = min_span;
        A.dhit = u->d_dhit.p; A.runs = u->d_runs.p; A.n_hits = (agx_u32)u->nh; A.n_runs = (agx_u32)u->n_runs; A.n_pos = n_pos; A.side_xpos = u->d_side_xpos.p;
        track_src[0] = A.c_pos; track_src[1] = V.c_depth; track_src[2] = V.c_step;
        return bytes;
    };
    C.whole = [&](const Export &E) {      // the whole unit's span and cross: a sub-window's start and end are its piece of the two arrays
        agx_u32 *const span_all = S.start, *const cross_all = S.end;
        n_passes = span_passes(E, S, 0, n_pos, sub, "walk span", [&](agx_u32 x) { S.start = span_all + x; S.end = cross_all + x; }, [](agx_u32, agx_u32) {}).passes;
    };
    C.gather = [&](const Export &E, agx_u32 n) {
        A.jt_cap = 0; A.n_ent = 0; A.n_list = 0;
        agx_launch_walk_span_gather(&A, E.s);
        agx_u32 nj = 0;
        E.read(&nj, A.joff + n, 4); E.sync();
        if (nj > n) throw Error{E_DEVICE, "internal: walk span: more jumps than bases"};
        if (nj) {
            A.jt_cap = nj;
            agx_launch_walk_span_emit(&A, E.s);
            agx_u32 *src[3] = {A.jt_x, A.jt_y, A.jt_base};
            for (int k = 0; k < 3; k++) { jt[k].resize(nj); E.read(jt[k].data(), src[k], (size_t)nj * 4); }
            agx_u32 w0 = 0;
            E.read(&w0, words, 4); E.sync();
            if (w0 || !span_jump_entries(jt[0].data(), jt[1].data(), jt[2].data(), nj, J)) throw Error{E_DEVICE, "internal: walk span: the jump list is inconsistent (error word " + std::to_string(w0) + ")"};
            const size_t ne = J.e_x.size();
            E.write(A.e_x, J.e_x.data(), ne * 4); E.write(A.e_y, J.e_y.data(), ne * 4); E.write(A.l_base, J.l_base.data(), (size_t)nj * 4); E.write(A.l_ent, J.l_ent.data(), (size_t)nj * 4);
            E.fill(A.e_cnt, 0, ne * 4);
            A.n_ent = (agx_u32)ne; A.n_list = nj;
            agx_launch_walk_span_jumps(&A, E.s);
            e->n_jump_steps += nj; n_entries += ne;
        }
        agx_launch_walk_span_flags(&A, E.s);
        n_chunks++;
    };
    records_body(u, w, F, tracks, rec_lo, rec_hi, O, V, C);
    if (g_trace) fprintf(stderr, "[agx trace] unit %p walk span (min %u): %u sub-windows, %u chunks of bases, %llu jump steps in %llu entries, %zu intervals\n", (void *)u, min_span, n_passes, n_chunks,
                         (unsigned long long)e->n_jump_steps, (unsigned long long)n_entries, (size_t)e->n_intervals);
    trace(u, "walk_span", t0, (size_t)F.total);
}

int agx_unit_walk_span(agx_unit *u, const agx_walk_paths *w, uint32_t min_span, uint32_t want_tracks, uint32_t rec_lo, uint32_t rec_hi, agx_walk_span *e) {
    return answer(u, e, agx_walk_span_free, w != nullptr, [&] { walk_span(u, *w, min_span, want_tracks != 0, rec_lo, rec_hi, e); });
}

void agx_walk_span_free(agx_walk_span *e) {
    if (!e) return;
    free(e->rec_graph_bases); free(e->rec_steps); free(e->rec_span_sum); free(e->rec_span_min); free(e->rec_span_min_at); free(e->rec_step_min); free(e->rec_step_min_at);
    free(e->iv_rec); free(e->iv_first); free(e->iv_last); free(e->iv_span_min); free(e->iv_step_min);
    free(e->track_off); free(e->pos); free(e->span); free(e->step);
    memset(e, 0, sizeof *e);
}

// Mate links: the table is checked and flattened as for the evidence and uploaded; own, the shadow count and the first pass over all hits (the per-record
// counters and the totals) go in one queue; every pass ends in one host round trip (the error and overflow words and the kept count) and, if it fit, a second (its links).
// Each pass is one more read of all hits: a table that fits the links needs one.
static void mate_links(agx_unit *u, const agx_walk_paths &w, uint32_t min_pairs, agx_mate_links *l) {
    const double t0 = now_ms();
    span_check(u, "mate links");
    const FlatTable F = check_walk_table(u, w, false, 0, 0, "mate links");
    const size_t nr = F.nr, ns = F.ns;
    size_t forced = 0;
    if (const char *env = getenv("AGX_LINKS_SLOTS")) {
        char *end = nullptr; const unsigned long long v = strtoull(env, &end, 10);
        if (!*env || *end || v < 2 || v > (1ull << 31) || (v & (v - 1))) throw Error{E_ARG, std::string("mate links: AGX_LINKS_SLOTS=") + env + " is not a power of two from 2 to 2^31"};
        forced = (size_t)v;
    }
    l->n_recs = (uint32_t)nr;
    host_array(l->rec_inside, nr); host_array(l->rec_open_left, nr); host_array(l->rec_open_right, nr); host_array(l->rec_links_out, nr); host_array(l->rec_links_in, nr);
    Export E(u);
    const agx_u32 n_pos = E.n_pos;
    E.open();
    const size_t avail = u->d_ut.n, parts = agx_links_partials((agx_u32)u->nh), sparts = agx_links_partials((agx_u32)std::max<uint64_t>(F.total, n_pos));
    auto bytes_of = [&](size_t slots) { return links_layout(ns, nr, n_pos, parts, sparts, slots, nullptr, nullptr); };
    // the natural size: twice the keys there can be at most — a key per hit, a key per ordered pair of records — as a power of two
    const unsigned long long most = std::min<unsigned long long>(u->nh, (unsigned long long)nr * (nr ? nr - 1 : 0));
    size_t slots = 2;
    while (slots < 2 * most && slots < ((size_t)1 << 31)) slots <<= 1;
    if (forced) slots = forced;
    else while (slots > 2 && bytes_of(slots) > avail) slots >>= 1;
    if (bytes_of(slots) > avail)
        throw Error{E_UNSUPPORTED, "mate links: own (" + std::to_string(n_pos) + " positions), the stretch table (" + std::to_string(ns) + " stretches, " + std::to_string(nr) + " records) and a table of " +
                                   std::to_string(slots) + " slots do not fit the export's scratch of " + std::to_string(avail) + " bytes"};
    agx_u32 log2_slots = 0; while (((size_t)1 << log2_slots) < slots) log2_slots++;
    agx_links_args A{};
    links_layout(ns, nr, n_pos, parts, sparts, slots, u->d_ut.p, &A);
    A.dhit = u->d_dhit.p; A.runs = u->d_runs.p; A.n_hits = (agx_u32)u->nh; A.n_runs = (agx_u32)u->n_runs; A.n_pos = n_pos; A.side_xpos = u->d_side_xpos.p;
    A.n_recs = (agx_u32)nr; A.min_pairs = min_pairs; A.slots = (agx_u32)slots; A.log2_slots = log2_slots;
    F.bind(E, A.T, nullptr, nullptr);
    std::vector<unsigned long long> keys, lens, g_key, g_len; std::vector<agx_u32> nums[5], g_num[5];      // n_pairs, lo_min, lo_max, hi_min, hi_max
    uint64_t distinct = 0;
    agx_u32 stuck = 0, stuck_dropped = 0;
    const long passes = links_plan((agx_u32)nr, [&](agx_u32 a_lo, agx_u32 a_hi, bool first) {
        A.a_lo = a_lo; A.a_hi = a_hi; A.count = first ? 1u : 0u; A.init_all = A.count;
        E.fill(A.words, 0, 32);
        if (first) { E.fill(A.part, 0, 6 * parts * 4); E.fill(A.spart, 0, 2 * sparts * 4); }
        agx_launch_links_init(&A, E.s);
        if (first) agx_launch_links_own(&A, E.s);
        agx_launch_links_pass(&A, E.s);
        agx_u32 wd[3] = {0, 0, 0}, kept = 0;
        E.read(wd, A.words, 12); E.read(&kept, A.off + slots, 4);
        E.sync();
        HIP_OK(hipGetLastError());
        if (wd[0]) throw Error{E_DEVICE, "internal: mate links: the owners or the kept slots are inconsistent (error word " + std::to_string(wd[0]) + ")"};
        if (wd[1]) { stuck_dropped = wd[1]; return false; }      // the pass is discarded
        if (wd[2] > slots || kept > wd[2]) throw Error{E_DEVICE, "internal: mate links: " + std::to_string(kept) + " kept of " + std::to_string(wd[2]) + " slots in use of " + std::to_string(slots)};
        distinct += wd[2];
        if (kept) {
            g_key.resize(kept); g_len.resize(kept);
            E.read(g_key.data(), A.o_key, (size_t)kept * 8); E.read(g_len.data(), A.o_len, (size_t)kept * 8);
            agx_u32 *src[5] = {A.o_n, A.o_lo_min, A.o_lo_max, A.o_hi_min, A.o_hi_max};
            for (int k = 0; k < 5; k++) { g_num[k].resize(kept); E.read(g_num[k].data(), src[k], (size_t)kept * 4); }
            E.sync();
            keys.insert(keys.end(), g_key.begin(), g_key.end()); lens.insert(lens.end(), g_len.begin(), g_len.end());
            for (int k = 0; k < 5; k++) nums[k].insert(nums[k].end(), g_num[k].begin(), g_num[k].end());
        }
        return true;
    }, &stuck);
    if (passes < 0)
        throw Error{E_UNSUPPORTED, "mate links: the links that leave record " + std::to_string(stuck) + " alone do not fit a table of " + std::to_string(slots) + " slots (" + std::to_string(stuck_dropped) +
                                   " pairs found none); the scratch holds no larger one"};
    {   // the counters and the totals: the first pass's, whether it fit or not — they never depended on the table, and the later passes added to none of them
        std::vector<agx_u32> part(6 * parts), spart(2 * sparts), rec(5 * nr + 1);
        E.read(part.data(), A.part, part.size() * 4); E.read(spart.data(), A.spart, spart.size() * 4);
        if (nr) E.read(rec.data(), A.rec, 5 * nr * 4);
        E.sync();
        uint64_t t[6] = {0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < parts; i++) for (int k = 0; k < 6; k++) t[k] += part[6 * i + k];
        for (size_t i = 0; i < sparts; i++) { l->n_shadowed += spart[2 * i]; l->n_owned += spart[2 * i + 1]; }
        l->n_kept = t[0]; l->n_outside = t[1]; l->n_fragments = t[0] - t[1]; l->n_unowned = t[2]; l->n_inside = t[3]; l->n_open = t[4]; l->n_link_pairs = t[5];
        if (t[1] > t[0] || t[2] + t[3] + t[4] + t[5] != l->n_fragments)
            throw Error{E_DEVICE, "internal: mate links: the classes (" + std::to_string(t[2]) + " + " + std::to_string(t[3]) + " + " + std::to_string(t[4]) + " + " + std::to_string(t[5]) +
                                  ") do not add up to the " + std::to_string(l->n_fragments) + " fragments"};
        uint32_t *dst[5] = {l->rec_inside, l->rec_open_left, l->rec_open_right, l->rec_links_out, l->rec_links_in};
        for (int k = 0; k < 5; k++) if (nr) memcpy(dst[k], rec.data() + k * nr, nr * 4);
    }
    const size_t nl = keys.size();
    if (nl >= 0xFFFFFFFFull) throw Error{E_UNSUPPORTED, "mate links: 2^32 links or more"};
    // the ranges are disjoint in A: sorting the concatenated lists by (A, B) is all the merge there is
    std::vector<size_t> order(nl);
    for (size_t i = 0; i < nl; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    for (size_t i = 1; i < nl; i++) if (keys[order[i - 1]] == keys[order[i]]) throw Error{E_DEVICE, "internal: mate links: a link came out of two slots"};
    l->n_links = (uint32_t)nl; l->n_links_all = distinct; l->n_passes = (uint32_t)passes; l->n_slots = (uint32_t)slots;
    host_array(l->a, nl); host_array(l->b, nl); host_array(l->n_pairs, nl); host_array(l->len_sum, nl); host_array(l->lo_min, nl); host_array(l->lo_max, nl); host_array(l->hi_min, nl); host_array(l->hi_max, nl);
    for (size_t i = 0; i < nl; i++) {
        const size_t j = order[i];
        l->a[i] = (uint32_t)(keys[j] >> 32); l->b[i] = (uint32_t)keys[j]; l->len_sum[i] = lens[j];
        l->n_pairs[i] = nums[0][j]; l->lo_min[i] = nums[1][j]; l->lo_max[i] = nums[2][j]; l->hi_min[i] = nums[3][j]; l->hi_max[i] = nums[4][j];
    }
    l->ms = now_ms() - t0;
    if (g_trace) fprintf(stderr, "[agx trace] unit %p mate links (min %u): %ld passes, %zu slots, %llu distinct keys, %zu kept links\n", (void *)u, min_pairs, passes, slots, (unsigned long long)distinct, nl);
    trace(u, "mate_links", t0, u->nh);
}

int agx_unit_mate_links(agx_unit *u, const agx_walk_paths *w, uint32_t min_pairs, agx_mate_links *l) {
    return answer(u, l, agx_mate_links_free, w != nullptr, [&] { mate_links(u, *w, min_pairs, l); });
}

void agx_mate_links_free(agx_mate_links *l) {
    if (!l) return;
    free(l->rec_inside); free(l->rec_open_left); free(l->rec_open_right); free(l->rec_links_out); free(l->rec_links_in);
    free(l->a); free(l->b); free(l->n_pairs); free(l->len_sum); free(l->lo_min); free(l->lo_max); free(l->hi_min); free(l->hi_max);
    memset(l, 0, sizeof *l);
}

// Bubbles: the region export's front as far as its phase 3 — the export's own round trips up to the totals —, then, where the tables lie: the in-degrees, the
// classes and the three scans (a round trip: the totals by class and the three counts), the rows (another: the table comes down).  No segment table is downloaded.
static void unit_bubbles(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, uint32_t max_nodes, bool support, agx_bubbles *b) {
    const double t0 = now_ms();
    b->max_nodes = max_nodes; b->has_support = support ? 1u : 0u;
    uint64_t n_bub = 0, n_rows = 0, n_bases = 0;
    PBuf<char> pin;
    size_t o_b = 0, o_r = 0, o_cov = 0, o_sup = 0, o_seq = 0;
    const ExportTail tail = [&](const Export &E, const agx_unitig_region_args &R, agx_u32 *words, agx_u32 ns, agx_u32 nb, agx_u32 nl) {
        const agx_unitig_args &X = R.U;
        b->n_segs = ns; b->n_links = nl;
        if (!ns) return;
        const size_t seg4 = 4 * (size_t)ns;
        Gaps take((char *)R.l_slot, u->d_ut.p + u->d_ut.n, {{X.s_hpos, seg4}, {X.s_hvar, seg4}, {X.s_last, seg4}, {X.s_len, seg4}, {X.s_cov, 2 * seg4}, {X.s_off, seg4 + 4}, {X.l_off, seg4 + 4},
                                                            {X.l_to, 4 * (size_t)nl}, {X.seq, nb}});
        agx_bubbles_args A{};
        A.s_hpos = X.s_hpos; A.s_hvar = X.s_hvar; A.s_last = X.s_last; A.s_len = X.s_len; A.s_off = X.s_off; A.l_off = X.l_off; A.l_to = X.l_to; A.s_cov = X.s_cov; A.seq = X.seq;
        A.l_sup = support && nl ? u->d_lsup.p : nullptr;
        A.n_segs = ns; A.n_links = nl; A.n_bases = nb; A.max_nodes = max_nodes; A.scan_tmp = X.scan_tmp; A.err = words; A.n_part = agx_bubbles_partials(ns);
        bubbles_layout(take, false, A);
        E.fill(A.s_in, 0, seg4 + 4);
        agx_launch_bubbles_class(&A, E.s);
        agx_u32 tot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, h[4] = {0, 0, 0, 0};
        E.read(tot, A.tot, 32); E.read(h, A.boff + ns, 4); E.read(h + 1, A.koff + ns, 4); E.read(h + 2, A.baoff + ns, 4); E.read(h + 3, words, 4); E.sync();
        HIP_OK(hipGetLastError());
        if (h[3] & ~16u) throw Error{E_DEVICE, "unitigs: the segments are inconsistent (error word " + std::to_string(h[3]) + ")"};
        if (h[3] || tot[7]) throw Error{E_DEVICE, "internal: bubbles: " + std::to_string(tot[7]) + " segments of the table the export left do not describe themselves (error word " + std::to_string(h[3]) + ")"};
        if ((uint64_t)tot[0] != (uint64_t)tot[1] + tot[2] + tot[3] + tot[4] + tot[5])
            throw Error{E_DEVICE, "internal: bubbles: " + std::to_string(tot[0]) + " forks, but their classes add up to " + std::to_string((uint64_t)tot[1] + tot[2] + tot[3] + tot[4] + tot[5])};
        b->n_forks = tot[0]; b->n_bubbles_all = tot[1]; b->n_tip = tot[2]; b->n_nested = tot[3]; b->n_sinks_differ = tot[4]; b->n_sink_shared = tot[5]; b->longest_branch = tot[6];
        if (h[0] > tot[1] || h[1] > nl || h[2] > nb || (h[0] && h[1] < 2ull * h[0])) throw Error{E_DEVICE, "internal: bubbles: the table's counts are out of range"};
        n_bub = h[0]; n_rows = h[1]; n_bases = h[2];
        if (!n_bub) return;
        A.bub_cap = h[0]; A.row_cap = h[1]; A.base_cap = h[2];
        bubbles_layout(take, true, A);
        agx_launch_bubbles_emit(&A, E.s);
        // the rows into pinned memory: six words per bubble, five per branch row and its coverage, the support on request, the bases
        o_r = o_b + 24 * (size_t)n_bub; o_cov = (o_r + 16 * (size_t)n_rows + 7) & ~(size_t)7; o_sup = o_cov + 8 * (size_t)n_rows; o_seq = o_sup + (A.l_sup ? 8 * (size_t)n_rows : 0);
        pin.alloc(o_seq + n_bases + 8);
        const agx_u32 *bsrc[6] = {A.b_spos, A.b_svar, A.b_slast, A.b_tpos, A.b_tvar, A.b_broff}, *rsrc[4] = {A.r_pos, A.r_var, A.r_nodes, A.r_seqoff};
        for (int i = 0; i < 6; i++) E.read(pin.p + o_b + 4 * (size_t)n_bub * i, bsrc[i], 4 * (size_t)n_bub);
        for (int i = 0; i < 4; i++) E.read(pin.p + o_r + 4 * (size_t)n_rows * i, rsrc[i], 4 * (size_t)n_rows);
        E.read(pin.p + o_cov, A.r_cov, 8 * (size_t)n_rows);
        if (A.l_sup) { E.read(pin.p + o_sup, A.r_in, 4 * (size_t)n_rows); E.read(pin.p + o_sup + 4 * (size_t)n_rows, A.r_out, 4 * (size_t)n_rows); }
        if (n_bases) E.read(pin.p + o_seq, A.o_seq, n_bases);
        E.read(h + 3, words, 4); E.sync();
        HIP_OK(hipGetLastError());
        if (h[3]) throw Error{E_DEVICE, "internal: bubbles: the rows disagree with their counts (error word " + std::to_string(h[3]) + ")"};
        b->bytes_down = 48 + o_seq + n_bases + 4;
    };
    agx_unitigs none{}; uint32_t *lsup = nullptr;
    region_export(u, pos_lo, pos_hi, min_coverage, &none, nullptr, support ? &lsup : nullptr, &tail);
    host_array(b->src_pos, n_bub); host_array(b->src_var, n_bub); host_array(b->src_last, n_bub); host_array(b->sink_pos, n_bub); host_array(b->sink_var, n_bub); host_array(b->br_off, n_bub);
    host_array(b->br_pos, n_rows); host_array(b->br_var, n_rows); host_array(b->br_nodes, n_rows); host_array(b->br_cov, n_rows); host_array(b->br_seq_off, n_rows); host_array(b->seq, n_bases);
    if (support) { host_array(b->br_sup_in, n_rows); host_array(b->br_sup_out, n_rows); }
    if (n_bub) {
        uint32_t *bdst[6] = {b->src_pos, b->src_var, b->src_last, b->sink_pos, b->sink_var, b->br_off}, *rdst[3] = {b->br_pos, b->br_var, b->br_nodes};
        for (int i = 0; i < 6; i++) memcpy(bdst[i], pin.p + o_b + 4 * (size_t)n_bub * i, 4 * (size_t)n_bub);
        for (int i = 0; i < 3; i++) memcpy(rdst[i], pin.p + o_r + 4 * (size_t)n_rows * i, 4 * (size_t)n_rows);
        const agx_u32 *so = (const agx_u32 *)(pin.p + o_r + 12 * (size_t)n_rows);
        for (size_t r = 0; r < n_rows; r++) b->br_seq_off[r] = so[r];
        memcpy(b->br_cov, pin.p + o_cov, 8 * (size_t)n_rows);
        if (support && b->n_links) { memcpy(b->br_sup_in, pin.p + o_sup, 4 * (size_t)n_rows); memcpy(b->br_sup_out, pin.p + o_sup + 4 * (size_t)n_rows, 4 * (size_t)n_rows); }
        memcpy(b->seq, pin.p + o_seq, n_bases);
        // what the kernels wrote must be a table: rows and bases in order, each bubble two rows at least
        for (size_t i = 0; i < n_bub; i++)
            if (b->br_off[i] > n_rows || (i && b->br_off[i] < b->br_off[i - 1] + 2u)) throw Error{E_DEVICE, "internal: bubbles: the branch offsets are inconsistent (bubble " + std::to_string(i) + ")"};
        for (size_t r = 0; r < n_rows; r++)
            if (b->br_seq_off[r] + b->br_nodes[r] != (r + 1 < n_rows ? b->br_seq_off[r + 1] : n_bases)) throw Error{E_DEVICE, "internal: bubbles: the base offsets are inconsistent (row " + std::to_string(r) + ")"};
    }
    b->br_off[n_bub] = (uint32_t)n_rows; b->br_seq_off[n_rows] = n_bases;
    b->n_bubbles = (uint32_t)n_bub; b->n_branches = (uint32_t)n_rows; b->n_bases = n_bases;
    b->ms = now_ms() - t0;
}

int agx_unit_bubbles(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, uint32_t max_nodes, uint32_t want_support, agx_bubbles *b) {
    return answer(u, b, agx_bubbles_free, true, [&] { unit_bubbles(u, pos_lo, pos_hi, min_coverage, max_nodes, want_support != 0, b); });
}

// Test hook (behind the primitives' hooks): overwrites what the calls above must not trust.  what & 1: every byte of the export's scratch, taken as
// Export::open() takes it, so that the call behind finds the buffer in place; what & 2: the edge counters, unless they hold the last build's counts (then they are state).
// pattern 0, 1, 2: bytes 0x00, 0xFF, 0xA5; 3: 32-bit words of a host xorshift of `seed`.  Memsets and one upload on the export's own stream, waited for; no kernel.
int agx_test_poison(agx_unit *u, uint32_t what, uint32_t pattern, uint64_t seed) {
    if (!u || pattern > 3u || (what & ~3u)) return AGX_E_ARG;
    return guarded(u, [&] {
        export_check(u, false, "test poison", "only such units reserve the export's scratch", "is poisoned");
        Export E(u);
        if (what & 1u) E.open(); else E.open_stream();
        uint64_t x = seed ? seed : 0x9E3779B97F4A7C15ull;
        std::vector<agx_u32> junk;
        auto poison = [&](void *p, size_t bytes) {
            if (!p || !bytes) return;
            if (pattern < 3u) { E.fill(p, pattern == 0u ? 0x00 : pattern == 1u ? 0xFF : 0xA5, bytes); return; }
            junk.resize((bytes + 3) / 4);
            for (agx_u32 &w : junk) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; w = (agx_u32)(x >> 16); }
            E.write(p, junk.data(), bytes); E.sync();      // (junk is filled again for the next array)
        };
        if (what & 1u) poison(u->d_ut.p, u->d_ut.n);
        if ((what & 2u) && (u->prm.flags & AGX_FLAG_EDGE_SUPPORT) && !u->support_valid) {
            poison(u->d_e_cnt.p, u->d_e_cnt.n * 4); poison(u->d_ovf_cnt.p, u->d_ovf_cnt.n * 4); poison(u->d_sup_tot.p, u->d_sup_tot.n * 4);
        }
        E.sync();
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
