// damaged_inputs_san.cpp — TEST-ONLY, a program of its own: what the content rules of the two binary doors (agx_host.h "content rules") let through.
//
//   damaged_inputs_san <tmp dir> <unit> <k> <mutants> <seed> [-v]
//
// tests/test_damaged_inputs.py compiles it together with the host loaders under the host sanitizers (-fsanitize=address,undefined) and runs it on one small unit that has
// every structure.  It makes the staged arrays of the unit's text in memory, then a seeded list of single-field mutants: the field uniform over all fields of all sections
// and the header's counts, the value out of {0, 1, bound - 1, bound, bound + 1, all ones, a random word}.  Per mutant both doors' checks are applied.  A mutant that either
// refuses is counted under the rule's name.  A mutant that both accept goes through everything that reads those arrays before and during a build, every array in a heap
// block of its own of exactly the element count the engine gives its device buffer (agx_engine.cpp: fixed_bufs), so that an index past an array is a sanitizer report:
//   * the host side: order_hits, the product's tile-ordered gather with the hits packed inside it (agx_forms.h: gather_tiled, HitPacker — what stage_tiled calls), the compact
//     hit and side packers through tests/wire_shim.cpp and their way back, build_row_diffs;
//   * the device's tables of the conti-mer runs the way its kernels fill them (agx_cm_layout_pos, agx_cm_fill_elem: agx_k_cm_fill's indexing) and the hop search over them;
//   * the serial executor (tests/hostsim): hit preparation with the span guard of agx_k_hit_prep, tile lists, every arrival of every listed hit through agx_decode_arrival /
//     agx_arrival_fetch (the vote-code and cm_head reads) inside the sweep's lane function, the edge lane functions, walk preparation, and the host walk with its k-mer tails.
// A refusal by a later, defined guard (E_ALIGNMENT, E_UNSUPPORTED / E_FORMAT "beyond the end of the unit", E_OVERFLOW, E_ARG) is a clean outcome.  A sanitizer report ends
// the program non-zero.  It prints the counts: refused per rule, accepted and clean, accepted and refused later.
#include "hostsim/agx_hostsim.cpp"
#include "wire_shim.cpp"

#include <map>
#include <random>

namespace {

template <class T> struct Exact {      // a heap block of exactly n elements
    std::unique_ptr<T[]> p; size_t n = 0;
    Exact() = default;
    explicit Exact(size_t count) : p(new T[count]()), n(count) {}
    Exact(const std::vector<T> &v, size_t count) : p(new T[count]()), n(count) { if (!v.empty()) memcpy(p.get(), v.data(), std::min(count, v.size()) * sizeof(T)); }
    T *get() const { return p.get(); }
};

struct Counts { unsigned long long nh, n_sides, n_runs, n_jump, n_other, n_rows, n_codes, n_pos, n_ref, n_cm, n_segs, n_seg0, n_chain_end, n_slots; agx_u32 stride, maxlen, slot_stride, rows_in_reads; };
struct Arrays {      // a unit's staged form: what both files carry
    std::vector<agx_whit> hits; std::vector<agx_wside> sides; std::vector<agx_wrun> runs; std::vector<agx_u32> jump; std::vector<unsigned long long> other; std::vector<agx_u8> codes;
    std::vector<agx_cmseg> segs; std::vector<agx_u8> cm_cnt; std::vector<agx_u32> chain_end, rows;
    Counts c;
};

enum Section { HITS, SIDES, RUNS, JUMP, OTHER, SEGS, CM_CNT, CHAIN_END, ROWS, COUNTS, N_SECTIONS };
struct Field { Section sec; const char *name; size_t off, width; };
#define F_OF(sec, T, f) Field{sec, #f, offsetof(T, f), sizeof(T::f)}
const Field FIELDS[] = {
    F_OF(HITS, agx_whit, a), F_OF(HITS, agx_whit, b), F_OF(HITS, agx_whit, row), F_OF(HITS, agx_whit, len), F_OF(HITS, agx_whit, flags), F_OF(HITS, agx_whit, back),
    F_OF(SIDES, agx_wside, runs1), F_OF(SIDES, agx_wside, runs2), F_OF(SIDES, agx_wside, nruns),
    F_OF(RUNS, agx_wrun, t), F_OF(RUNS, agx_wrun, q), F_OF(RUNS, agx_wrun, n),
    Field{JUMP, "entry", 0, 4}, Field{OTHER, "entry", 0, 8},
    F_OF(SEGS, agx_cmseg, pos0), F_OF(SEGS, agx_cmseg, len), F_OF(SEGS, agx_cmseg, cid), F_OF(SEGS, agx_cmseg, coff0), F_OF(SEGS, agx_cmseg, dcoff), F_OF(SEGS, agx_cmseg, rank),
    F_OF(SEGS, agx_cmseg, hop_str0), F_OF(SEGS, agx_cmseg, hop_len0), F_OF(SEGS, agx_cmseg, hop_end), F_OF(SEGS, agx_cmseg, elem0),
    Field{CM_CNT, "count", 0, 1}, Field{CHAIN_END, "entry", 0, 4}, Field{ROWS, "slot", 0, 4},
    F_OF(COUNTS, Counts, nh), F_OF(COUNTS, Counts, n_sides), F_OF(COUNTS, Counts, n_runs), F_OF(COUNTS, Counts, n_jump), F_OF(COUNTS, Counts, n_other), F_OF(COUNTS, Counts, n_rows),
    F_OF(COUNTS, Counts, n_codes), F_OF(COUNTS, Counts, n_pos), F_OF(COUNTS, Counts, n_ref), F_OF(COUNTS, Counts, n_cm), F_OF(COUNTS, Counts, n_segs), F_OF(COUNTS, Counts, n_seg0),
    F_OF(COUNTS, Counts, n_chain_end), F_OF(COUNTS, Counts, n_slots), F_OF(COUNTS, Counts, stride), F_OF(COUNTS, Counts, maxlen), F_OF(COUNTS, Counts, slot_stride), F_OF(COUNTS, Counts, rows_in_reads),
};
const size_t N_FIELDS = sizeof FIELDS / sizeof FIELDS[0];

struct SectionRef { char *p; size_t elem, count; };
SectionRef section_of(Arrays &A, Section s) {
    switch (s) {
    case HITS: return {(char *)A.hits.data(), sizeof(agx_whit), A.hits.size()};
    case SIDES: return {(char *)A.sides.data(), sizeof(agx_wside), A.sides.size()};
    case RUNS: return {(char *)A.runs.data(), sizeof(agx_wrun), A.runs.size()};
    case JUMP: return {(char *)A.jump.data(), 4, A.jump.size()};
    case OTHER: return {(char *)A.other.data(), 8, A.other.size()};
    case SEGS: return {(char *)A.segs.data(), sizeof(agx_cmseg), A.segs.size()};
    case CM_CNT: return {(char *)A.cm_cnt.data(), 1, A.cm_cnt.size()};
    case CHAIN_END: return {(char *)A.chain_end.data(), 4, A.chain_end.size()};
    case ROWS: return {(char *)A.rows.data(), 4, A.rows.size()};
    default: return {(char *)&A.c, sizeof(Counts), 1};
    }
}
unsigned long long get_field(const char *p, size_t w) { unsigned long long v = 0; memcpy(&v, p, w); return v; }

// the value a field's natural partner bounds it by (element e of the intact unit)
unsigned long long bound_of(const Arrays &A, const Field &f, size_t e) {
    const Counts &c = A.c; const std::string n = f.name;
    switch (f.sec) {
    case HITS: { const agx_whit &w = A.hits[e];
        if (n == "a") return (w.flags & AGX_WF_RUNS1) ? c.n_sides : c.n_pos;
        if (n == "b") return (!(w.flags & AGX_WF_RUNS1) && (w.flags & AGX_WF_RUNS2)) ? c.n_sides : c.n_pos;
        return n == "row" ? c.n_rows : n == "len" ? c.maxlen : n == "flags" ? 64 : e; }
    case SIDES: return n == "nruns" ? 0x10000 : c.n_runs;
    case RUNS: return n == "t" ? c.n_pos : c.maxlen;
    case JUMP: return c.nh;
    case OTHER: return c.n_rows * c.stride;
    case SEGS: return n == "rank" ? A.cm_cnt[A.segs[e].pos0] : n == "hop_str0" || n == "hop_len0" ? 64 : n == "elem0" ? c.n_cm : c.n_pos;
    case CM_CNT: return 255;
    case CHAIN_END: return c.n_pos;
    case ROWS: return c.n_slots;
    default: return get_field((const char *)&c + f.off, f.width);
    }
}

struct Verdict { const char *rule = nullptr; };
const char *both_checks(const Arrays &M, const Arrays &intact, size_t chain_str_len) {
    const Counts &c = M.c;
    {   // the headers both files would carry: the counts as they are now, the sections as long as they are
        pairsfile::Header P; memset(&P, 0, sizeof P); memcpy(P.magic, pairsfile::MAGIC, 8); P.version = 1; P.k = 5; P.batch = 1000000; P.stride = c.stride; P.maxlen = c.maxlen; P.n_rows = (agx_u32)c.n_rows;
        P.nh = c.nh; P.n_sides = c.n_sides; P.n_runs = c.n_runs; P.n_codes = c.n_codes; P.n_other = c.n_other; P.n_jump = c.n_jump; P.sizes[0] = sizeof(agx_whit); P.sizes[1] = sizeof(agx_wside); P.sizes[2] = sizeof(agx_wrun);
        const Counts &i = intact.c;
        const unsigned long long plen[pairsfile::S_N] = {i.nh * sizeof(agx_whit), i.n_sides * sizeof(agx_wside), i.n_runs * sizeof(agx_wrun), i.n_codes, i.n_other * 8, i.n_other, i.n_jump * 4};
        unsigned long long at = 4096; for (int s = 0; s < pairsfile::S_N; s++) { P.off[s] = at; P.len[s] = plen[s]; at = (at + plen[s] + 4095) & ~4095ull; }
        if (c.n_rows >= 0x7FFFFFFFull) return "count_limits";      // (the pairs file's n_rows is 32 bits wide)
        if (const char *r = pairs_header_rule(P, at)) return r;
        using namespace cachefile;
        Header H; memset(&H, 0, sizeof H); memcpy(H.magic, MAGIC, 8); H.version = 2; H.batch = 1000000; H.k = 5;
        H.n_pos = c.n_pos; H.n_ref = c.n_ref; H.nh = c.nh; H.n_runs = c.n_runs; H.n_cm = c.n_cm; H.n_segs = c.n_segs; H.n_seg0 = c.n_seg0; H.n_rows = c.n_rows; H.n_chain_end = c.n_chain_end; H.n_codes = c.n_codes;
        H.stride = c.stride; H.maxlen = c.maxlen; H.n_slots = (agx_u32)c.n_slots; H.rows_in_reads = c.rows_in_reads; H.slot_stride = c.slot_stride; H.n_sides = c.n_sides; H.n_jump = c.n_jump;
        H.sizes[0] = sizeof(agx_whit); H.sizes[1] = sizeof(agx_wrun); H.sizes[2] = sizeof(agx_cmseg); H.sizes[3] = sizeof(Header); H.sizes[4] = sizeof(agx_wside);
        const unsigned long long clen[S_N] = {i.nh * sizeof(agx_whit), i.n_runs * sizeof(agx_wrun), i.n_codes, i.n_segs * sizeof(agx_cmseg), i.n_chain_end * 4, i.n_rows * 4, i.n_pos, i.n_pos, chain_str_len, 0,
                                              i.n_slots * i.slot_stride, i.n_other * 8, i.n_sides * sizeof(agx_wside), i.n_jump * 4, 0};
        at = 4096; for (int s = 0; s < S_N; s++) { H.off[s] = at; H.len[s] = clen[s]; at = (at + clen[s] + 4095) & ~4095ull; }
        if (const char *r = cache_header_rule(H, at, 1000000, 5)) return r;
    }
    StagedView V; V.hits = M.hits.data(); V.nh = c.nh; V.sides = M.sides.data(); V.n_sides = c.n_sides; V.runs = M.runs.data(); V.n_runs = c.n_runs; V.jump = M.jump.data(); V.n_jump = c.n_jump;
    V.other = M.other.data(); V.n_other = c.n_other; V.n_rows = c.n_rows; V.stride = c.stride; V.maxlen = c.maxlen; V.n_pos = c.n_pos;
    if (const char *r = staged_pairs_rule(V, 2)) return r;
    if (const char *r = other_ascending_rule(V.other, V.n_other)) return r;      // (the pairs file's door, and a cache made of one)
    CacheView C; C.segs = M.segs.data(); C.n_segs = c.n_segs; C.cm_cnt = M.cm_cnt.data(); C.chain_end = M.chain_end.data(); C.n_chain_end = c.n_chain_end; C.rows = M.rows.data();
    C.n_pos = c.n_pos; C.n_cm = c.n_cm; C.n_rows = c.n_rows; C.chain_str_len = chain_str_len; C.reads_size = 0; C.maxlen = c.maxlen; C.n_slots = (agx_u32)c.n_slots; C.rows_in_reads = c.rows_in_reads;
    return cache_content_rule(C, 2);
}

struct Base { Threads T; std::vector<agx_u32> wref; bool ref_packed = false; };

// Everything that reads the staged arrays before and during a build.  Throws Error where a defined guard refuses the unit.
void consume(const Arrays &M, const Base &B, agx_u32 k) {
    const Counts &c = M.c;
    const size_t nh = (size_t)c.nh, n_pos = (size_t)c.n_pos, s4 = c.stride / 4, n_rows = (size_t)c.n_rows, n_tiles = (n_pos + AGX_TILE - 1) / AGX_TILE;
    // the arrays in blocks of the device buffers' element counts (fixed_bufs: d_whits nh + 1, d_wsides n_sides + 1, d_wruns n_runs + 1, d_jump n_jump + 1, d_other n + 1, d_codes bytes + 16)
    Exact<agx_whit> hits(M.hits, nh + 1); Exact<agx_wside> sides(M.sides, (size_t)c.n_sides + 1); Exact<agx_wrun> runs(M.runs, (size_t)c.n_runs + 1); Exact<agx_u32> jump(M.jump, (size_t)c.n_jump + 1);
    Exact<unsigned long long> other(M.other, (size_t)c.n_other + 1); Exact<agx_u8> codes(M.codes, (size_t)c.n_codes + 16);
    // ---- host: the tile order, the gather into it, the compact records, the rows against the reference
    Exact<agx_u32> perm(nh + 1), tile_first(n_tiles + 2), jump_at((size_t)c.n_jump + 1);
    order_hits(hits.get(), nh, sides.get(), runs.get(), jump.get(), (size_t)c.n_jump, n_pos, 2, perm.get(), tile_first.get(), jump_at.get());
    Exact<agx_whit> hits_t(nh + 1); Exact<agx_u8> codes_t(nh * s4 + 16); Exact<agx_u32> slot_row(nh); Exact<char> wire((nh + 1) * sizeof(agx_whit));
    HitWire fused{};      // what the packer inside the gather made, for the comparison below
    {   // the product's gather with the hits packed inside it (agx_forms.h: gather_tiled, HitPacker), as stage_tiled runs it, into blocks of the engine's element counts
        StagedView V; V.hits = hits.get(); V.nh = nh; V.sides = sides.get(); V.n_sides = (size_t)c.n_sides; V.runs = runs.get(); V.n_runs = (size_t)c.n_runs; V.other = other.get(); V.n_other = (size_t)c.n_other;
        V.n_rows = c.n_rows; V.stride = c.stride; V.maxlen = c.maxlen; V.n_pos = c.n_pos;
        HitPacker packer(nh, c.maxlen, 2, true);
        if (packer.on) packer.into(wire.get());
        (void)gather_tiled(V, codes.get(), perm.get(), 2, packer, hits_t.get(), codes_t.get(), slot_row.get());
        fused = packer.finish();
    }
    if (nh) {      // the compact records and the way back (agx_forms.h: HitPacker, plan_sides / fill_sides; agx_k_expand_hits, agx_k_side_*)
        Exact<agx_chit_block> blocks(nh / 64 + 1); Exact<agx_whit> esc(nh + 1), back(nh + 1); Exact<uint32_t> ext(nh + 1); uint32_t counts[2];
        agx_wire_pack_hits(hits_t.get(), (uint32_t)nh, c.maxlen, 2, blocks.get(), esc.get(), ext.get(), counts);
        agx_wire_unpack_hits(blocks.get(), (uint32_t)nh, c.maxlen, esc.get(), ext.get(), back.get());
        if (memcmp(back.get(), hits_t.get(), nh * sizeof(agx_whit)) != 0) throw Error{E_DEVICE, "compact hit records do not come back"};
        // the blocks packed inside the gather (where they gained and were laid out) are the blocks packed over its finished array: both on two threads
        if (fused.gain && (fused.n_esc != counts[0] || fused.n_ext != counts[1] || memcmp(wire.get(), blocks.get(), fused.n_blocks * sizeof(agx_chit_block)) != 0 ||
                           memcmp(fused.esc, esc.get(), fused.n_esc * sizeof(agx_whit)) != 0 || memcmp(fused.ext, ext.get(), fused.n_ext * 4) != 0))
            throw Error{E_DEVICE, "the blocks packed inside the gather differ from the blocks packed over its result"};
        const size_t ns = (size_t)c.n_sides;
        Exact<uint16_t> cc(ns + 4); Exact<agx_cside_esc> listed(ns + 1); Exact<agx_wside> sback(ns + 1); uint32_t n_listed = 0, first = 0;
        if (ns && agx_wire_pack_sides(sides.get(), (uint32_t)ns, cc.get(), listed.get(), &n_listed, &first)) {
            agx_wire_unpack_sides(cc.get(), (uint32_t)ns, listed.get(), n_listed, first, sback.get());
            for (size_t i = 0; i < ns; i++) {      // (a side's first run comes back for the mates that have runs)
                const agx_wside &a = sides.get()[i], &b = sback.get()[i];
                if (a.nruns != b.nruns || ((a.nruns & 0xFFFFu) && a.runs1 != b.runs1) || ((a.nruns >> 16) && a.runs2 != b.runs2)) throw Error{E_DEVICE, "compact side records do not come back"};
            }
        }
    }
    if (B.ref_packed && nh) { RowDiffs D; (void)build_row_diffs(hits_t.get(), nh, sides.get(), (size_t)c.n_sides, runs.get(), (size_t)c.n_runs, codes_t.get(), nh, c.stride, B.wref.data(), n_pos, 2, D, true); }
    // ---- the device's conti-mer tables out of the runs and the counts (agx_k_cm_layout, agx_k_cm_fill), and the hop search over the runs
    {
        Exact<agx_cmseg> segs(M.segs, (size_t)c.n_segs + 1); Exact<agx_u8> cnt(M.cm_cnt, n_pos);
        CmLayout L; build_cm_layout(cnt.get(), n_pos, segs.get(), (size_t)c.n_segs, L);
        Exact<agx_u32> start(n_pos + 2); Exact<agx_cmkey> cm((size_t)c.n_cm + 1); Exact<agx_cmhead> head(n_pos + 1);
        for (const agx_chunk &ch : L.cnt_chunks) { const agx_cntrun &r = L.cnt_runs[ch.run]; const agx_u32 n = std::min<agx_u32>(r.len - ch.off, AGX_CM_CHUNK); for (agx_u32 j = 0; j < n; j++) agx_cm_layout_pos(r, ch.off + j, start.get(), head.get()); }
        start.get()[n_pos] = (agx_u32)c.n_cm; head.get()[n_pos] = agx_cmhead{AGX_NONE, AGX_NONE, 0u, 0u};
        for (const agx_chunk &ch : L.seg_chunks) { const agx_cmseg &g = segs.get()[ch.run]; const agx_u32 n = std::min<agx_u32>(g.len - ch.off, AGX_CM_CHUNK); for (agx_u32 j = 0; j < n; j++) agx_cm_fill_elem(g, ch.off + j, start.get(), cm.get(), head.get()); }
        std::vector<agx_u32> index; build_seg_index(segs.get(), (size_t)c.n_seg0, n_pos, index);
        Exact<char> chain(B.T.chain_str.size() + 1); if (!B.T.chain_str.empty()) memcpy(chain.get(), B.T.chain_str.data(), B.T.chain_str.size());
        unsigned long long sum = 0;
        for (agx_u32 x = 0; x < n_pos; x++) {
            const agx_hop h = agx_seg_hop<agx_hop>(segs.get(), (agx_u32)c.n_seg0, start.get(), x);
            if (h.len) { if (h.end_pos >= n_pos) throw Error{E_DEVICE, "a hop ends beyond the unit"}; for (agx_u32 j = 0; j < h.len; j++) sum += (unsigned char)chain.get()[(size_t)h.str_off + j]; }
        }
        for (size_t i = 0; i < c.n_chain_end; i++) sum += head.get()[M.chain_end[i]].n;      // (agx_k_assign_aid marks a_mark[position])
        if (sum == ~0ull) fprintf(stderr, "(unreachable)\n");
    }
    // ---- the serial executor on the staged arrays: hit preparation, tile lists, sweep, edges, walk preparation, the walk
    {
        Threads T = B.T;      // (the loader's own tables of the intact text: the executor compares its expansions of T.segs with them, so the runs stay the text's here)
        Pairs P; P.stride = c.stride; P.n_slots = (agx_u32)n_rows;
        P.hits.resize(nh); std::vector<agx_u8> left(nh + 1);
        for (size_t h = 0; h < nh; h++) { P.hits[h] = agx_unpack_hit(hits.get()[h], sides.get()); left[h] = (agx_u8)(P.hits[h].pad[0] & 1u); }
        P.runs.resize((size_t)c.n_runs); for (size_t i = 0; i < c.n_runs; i++) P.runs[i] = agx_run{runs.get()[i].q, runs.get()[i].t, runs.get()[i].n};
        P.bases.assign(n_rows * c.stride + 16, 'A');      // (d_vcodes: packed bytes * 4 + 16)
        for (size_t i = 0; i < n_rows * c.stride; i++) P.bases[i] = "ACGT"[(codes.get()[i >> 2] >> (2u * (i & 3u))) & 3u];
        for (size_t j = 0; j < c.n_other; j++) P.bases[(size_t)other.get()[j]] = 'N';
        P.bases.shrink_to_fit(); P.hits.shrink_to_fit(); P.runs.shrink_to_fit();
        SimGraph S; int nbig = 0; SimOptions opt; SimRecords R; SimEdges E; SimFront F; opt.staged_left = left.data();
        simulate(T, P, k, 50, 4, AGX_MAXV_LDS, S, nbig, opt, R, E, F);
        GraphView G; G.n_pos = (agx_u32)T.ref.size(); G.n_ids = S.n_ids;
        G.meta = S.a_meta.data(); G.str = S.a_str.data(); G.side_xpos = S.side_xpos.data();
        G.sp_bits = S.sp_bits.data(); G.sp_rank = S.sp_rank.data(); G.sp_node = S.sp_node.data(); G.sp_hop = S.sp_hop.data(); G.n_special = S.n_special;
        G.fetch = [](void *ctx, agx_u32 first, agx_u32 stride, agx_u32 rows, agx_u32 width, agx_walknode *o) {
            for (agx_u32 r = 0; r < rows; r++) for (agx_u32 cc = 0; cc < width; cc++) { const SimGraph *g = (const SimGraph *)ctx; const size_t a = (size_t)first + (size_t)r * stride + cc; if (a >= g->n_ids) throw Error{E_ARG, "record fetch beyond the walk graph"}; o[(size_t)r * width + cc] = agx_walk_record(g->walk_args, (agx_u32)a); }
        }; G.fetch_ctx = &S;
        G.ovf = S.a_ovf.data(); G.n_ovf = S.ovf.size();
        UnitOutput O; walk_join_scaffold(view_of(T, P), G, O, nullptr);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: damaged_inputs_san <tmp dir> <unit> <k> <mutants> <seed>\n"); return 2; }
    const std::string d = argv[1], s = argv[2]; const agx_u32 k = (agx_u32)atoi(argv[3]); const long n_mut = atol(argv[4]); const unsigned seed = (unsigned)atol(argv[5]);
    Base B; Arrays A;
    try {
        load_unit_reference(d + "/_genome." + s + ".fa", B.T.ref);
        thread_contigs_from_files(d + "/_contigs.fa", d + "/_contigs_genome." + s + ".psl", B.T);
        VecSink sink; Pairs P; StagedPairs S;
        load_pairs_from_files(d + "/_reads.fa", d + "/_reads_genome." + s + ".bowtie", 1000000, k, P, nullptr);
        stage_pairs(P, k, 2, sink, S);
        A.hits.assign(S.hits, S.hits + S.nh); A.sides.assign(S.sides, S.sides + S.n_sides); A.runs.assign(S.runs, S.runs + S.n_runs); A.jump.assign(S.jump, S.jump + S.n_jump);
        A.other.assign(S.other, S.other + S.n_other); A.codes.assign(S.codes, S.codes + S.n_codes); A.segs = B.T.segs; A.cm_cnt = B.T.cm_cnt; A.rows = S.row_slot;
        A.chain_end = B.T.chain_end_pos; std::sort(A.chain_end.begin(), A.chain_end.end()); A.chain_end.erase(std::unique(A.chain_end.begin(), A.chain_end.end()), A.chain_end.end());
        A.c = Counts{S.nh, S.n_sides, S.n_runs, S.n_jump, S.n_other, S.n_rows, S.n_codes, B.T.ref.size(), B.T.n_ref, B.T.n_cm, B.T.segs.size(), B.T.n_seg0, A.chain_end.size(), P.n_slots, S.stride, S.maxlen, P.stride, 0u};
        std::vector<agx_u8> packed((B.T.ref.size() + 3) / 4 + 64, 0); std::vector<agx_refx> others;
        B.ref_packed = pack_reference(B.T.ref.data(), B.T.ref.size(), 2, packed.data(), others);
        B.wref.assign(packed.size() / 4 + 1, 0); memcpy(B.wref.data(), packed.data(), packed.size());
    } catch (const Error &e) { fprintf(stderr, "cannot load the unit: %s\n", e.msg.c_str()); return 2; }
    // the unit has every structure
    size_t n_back = 0, n_left2 = 0, n_rev = 0; for (const agx_whit &w : A.hits) { n_back += w.back != 0; n_left2 += (w.flags & AGX_WF_LEFT2) != 0; n_rev += (w.flags & AGX_WF_REV1) != 0; }
    if (A.sides.empty() || A.runs.empty() || A.jump.empty() || A.other.empty() || !n_back || !n_left2 || n_left2 == A.hits.size() || !n_rev || n_rev == A.hits.size() || A.segs.size() < 2 || A.chain_end.empty()) {
        fprintf(stderr, "the unit lacks a structure: %zu sides, %zu runs, %zu jump entries, %zu other bases, %zu hits with back, %zu of %zu with mate 2 left, %zu runs of conti-mers\n",
                A.sides.size(), A.runs.size(), A.jump.size(), A.other.size(), n_back, n_left2, A.hits.size(), A.segs.size());
        return 3;
    }
    // the intact unit is accepted and runs clean
    if (const char *r = both_checks(A, A, B.T.chain_str.size())) { fprintf(stderr, "the intact unit is refused: %s\n", r); return 4; }
    try { consume(A, B, k); } catch (const Error &e) { fprintf(stderr, "the intact unit does not run clean: %s\n", e.msg.c_str()); return 4; }
    printf("intact: accepted, clean\n");
    std::mt19937_64 rnd(seed);
    std::map<std::string, long> refused, later; long clean = 0;
    for (long m = 0; m < n_mut; m++) {
        Arrays M = A;
        const Field &f = FIELDS[rnd() % N_FIELDS];
        SectionRef sec = section_of(M, f.sec);
        if (!sec.count) continue;
        const size_t e = (size_t)(rnd() % sec.count);
        const unsigned long long bound = bound_of(A, f, e), all = f.width == 8 ? ~0ull : (1ull << (8 * f.width)) - 1;
        const unsigned long long choice[7] = {0, 1, bound - 1, bound, bound + 1, all, rnd()};
        const unsigned long long v = choice[rnd() % 7] & all;
        memcpy(sec.p + e * sec.elem + f.off, &v, f.width);
        const char *rule = both_checks(M, A, B.T.chain_str.size());
        if (rule) { refused[rule]++; continue; }
        if (argc > 6) fprintf(stderr, "mutant %ld: %s of element %zu of section %d = %llu\n", m, f.name, e, (int)f.sec, v);      // (any seventh argument: say which mutant runs, for a report to name)
        try { consume(M, B, k); clean++; }
        catch (const Error &err) {
            if (err.code == E_DEVICE) { fprintf(stderr, "mutant %ld (%s of element %zu = %llu): %s\n", m, f.name, e, v, err.msg.c_str()); return 5; }
            later[std::to_string(err.code) + " " + err.msg]++;
        }
    }
    long n_ref = 0; for (auto &r : refused) { printf("refused %s: %ld\n", r.first.c_str(), r.second); n_ref += r.second; }
    long n_later = 0; for (auto &r : later) { printf("accepted, refused later (%s): %ld\n", r.first.c_str(), r.second); n_later += r.second; }
    printf("mutants %ld: refused %ld, accepted and clean %ld, accepted and refused later %ld\n", n_mut, n_ref, clean, n_later);
    return 0;
}
