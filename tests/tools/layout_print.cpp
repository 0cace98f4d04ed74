// layout_print.cpp — a host-only program that prints what the export's layouts carve, for a grid of arguments: evidence_layout, walk_span_layout, links_layout, span_layout,
// edge_reads_layout, unitig_layout, unitig_region_layout, idmap_layout and mapped_scratch.  Per line: the size with base == nullptr and with a base, the offset of the
// words, and a hash of every pointer and capacity the layout filled in.  It includes the source file that holds the layouts (LAYOUT_SOURCE), so the output of two trees
// can be compared byte for byte after a change that must leave every offset where it was.  No device is touched and nothing of the included file is called but the
// layouts, so what they do not need stays unresolved.  From the repository root:
//   g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -DLAYOUT_SOURCE='"../../aligngraph_amd/csrc/agx_export.cpp"' -no-pie -Wl,-z,lazy \
//       -Wl,--unresolved-symbols=ignore-all -o layout_print tests/tools/layout_print.cpp && ./layout_print > layouts.txt
#include LAYOUT_SOURCE

static char *const BASE = (char *)(uintptr_t)0x100000000000ull;      // (never read or written: the layouts only add to it)

template <class A> static unsigned long long hash_of(const A &a) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char *p = (const unsigned char *)&a;
    for (size_t i = 0; i < sizeof a; i++) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
// an argument struct with every byte cleared, padding included
template <class A> struct Cleared { A a; Cleared() { memset((void *)&a, 0, sizeof a); } };

static void line(const char *name, const std::vector<size_t> &args, size_t size0, size_t size1, const agx_u32 *words, unsigned long long h) {
    printf("%s(", name);
    for (size_t i = 0; i < args.size(); i++) printf(i ? ", %zu" : "%zu", args[i]);
    printf("): %zu %zu words@%lld hash %016llx\n", size0, size1, words ? (long long)((const char *)words - BASE) : -1ll, h);
}

int main() {
    const std::vector<size_t> counts = {0, 1, 2, 63, 64, 65, 1000, 70001}, steps = {1, 64, 100, 4097};
    for (size_t cap : counts) for (size_t n_pos : counts) for (size_t n_ovf : counts) {
        { Cleared<agx_unitig_args> A; agx_u32 *w = nullptr;
          const size_t s0 = unitig_layout(cap, n_pos, n_ovf, nullptr, nullptr, nullptr), s1 = unitig_layout(cap, n_pos, n_ovf, BASE, &A.a, &w);
          line("unitig_layout", {cap, n_pos, n_ovf}, s0, s1, w, hash_of(A.a)); }
        for (size_t n_win : {(size_t)0, (size_t)1, n_pos / 2, n_pos}) for (size_t kept : {(size_t)0, (size_t)1, cap / 3, cap}) {
            Cleared<agx_unitig_region_args> R; agx_u32 *w = nullptr;
            const size_t s0 = unitig_region_layout(cap, n_win, kept, n_ovf, nullptr, nullptr, nullptr), s1 = unitig_region_layout(cap, n_win, kept, n_ovf, BASE, &R.a, &w);
            line("unitig_region_layout", {cap, n_win, kept, n_ovf}, s0, s1, w, hash_of(R.a));
        }
        for (size_t n_nodes : {(size_t)0, (size_t)1, cap, 2 * cap}) for (size_t n_ids : {(size_t)0, n_pos, n_pos + cap}) {
            size_t at = 0;
            const size_t s = mapped_scratch(cap, n_pos, n_nodes, n_ids, n_ovf, &at);
            line("mapped_scratch", {cap, n_pos, n_nodes, n_ids, n_ovf}, s, at, nullptr, 0);
        }
    }
    for (size_t ids : counts) for (size_t runs : counts) {
        Cleared<agx_idmap_args> M;
        const size_t s0 = idmap_layout(ids, runs, nullptr, nullptr), s1 = idmap_layout(ids, runs, BASE, &M.a);
        line("idmap_layout", {ids, runs}, s0, s1, nullptr, hash_of(M.a));
    }
    for (size_t n_st : counts) for (size_t n_recs : counts) for (size_t chunk : steps) {
        for (int tracks = 0; tracks < 2; tracks++) {
            Cleared<agx_evidence_args> A; agx_u32 *w = nullptr;
            const size_t s0 = evidence_layout(n_st, n_recs, chunk, tracks != 0, nullptr, nullptr, nullptr), s1 = evidence_layout(n_st, n_recs, chunk, tracks != 0, BASE, &A.a, &w);
            line("evidence_layout", {n_st, n_recs, chunk, (size_t)tracks}, s0, s1, w, hash_of(A.a));
        }
        for (size_t n_pos : {(size_t)0, (size_t)1, (size_t)70001}) for (size_t sub : steps) for (size_t parts : {(size_t)0, (size_t)1, (size_t)300}) {
            Cleared<agx_walk_span_args> A; Cleared<agx_span_args> S; agx_u32 *w = nullptr;
            const size_t s0 = walk_span_layout(n_st, n_recs, n_pos, sub, chunk, parts, nullptr, nullptr, nullptr, nullptr), s1 = walk_span_layout(n_st, n_recs, n_pos, sub, chunk, parts, BASE, &A.a, &S.a, &w);
            line("walk_span_layout", {n_st, n_recs, n_pos, sub, chunk, parts}, s0, s1, w, hash_of(A.a) ^ (hash_of(S.a) * 31));
        }
    }
    for (size_t n_st : counts) for (size_t n_recs : counts) for (size_t n_pos : {(size_t)0, (size_t)1, (size_t)70001}) for (size_t parts : {(size_t)0, (size_t)1, (size_t)300})
        for (size_t sparts : {(size_t)0, (size_t)1, (size_t)77}) for (size_t slots : {(size_t)0, (size_t)1, (size_t)2, (size_t)64, (size_t)65536}) {
            Cleared<agx_links_args> A;
            const size_t s0 = links_layout(n_st, n_recs, n_pos, parts, sparts, slots, nullptr, nullptr), s1 = links_layout(n_st, n_recs, n_pos, parts, sparts, slots, BASE, &A.a);
            line("links_layout", {n_st, n_recs, n_pos, parts, sparts, slots}, s0, s1, A.a.words, hash_of(A.a));
        }
    for (size_t sub : {(size_t)0, (size_t)1, (size_t)64, (size_t)100, (size_t)70001}) for (size_t parts : {(size_t)0, (size_t)1, (size_t)300}) {
        Cleared<agx_span_args> S;
        const size_t s0 = span_layout(sub, parts, nullptr, nullptr), s1 = span_layout(sub, parts, BASE, &S.a);
        line("span_layout", {sub, parts}, s0, s1, nullptr, hash_of(S.a));
    }
    for (size_t tiles : {(size_t)0, (size_t)1, (size_t)2, (size_t)1000}) for (size_t recs : counts) {
        Cleared<agx_reads_kargs> K; agx_u32 *w = nullptr;
        const size_t s0 = edge_reads_layout(tiles, recs, nullptr, nullptr, nullptr), s1 = edge_reads_layout(tiles, recs, BASE, &K.a, &w);
        line("edge_reads_layout", {tiles, recs}, s0, s1, w, hash_of(K.a));
    }
    return 0;
}
