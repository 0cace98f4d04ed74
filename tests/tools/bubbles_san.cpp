// bubbles_san.cpp — a stand-alone program for a sanitizer run of the host-side pieces of the bubbles on the CPU: the lane function
// (agx_bubble_class, the one the kernels call), the host-only twin (agx_unitigs_bubbles) and the TSV formatter (agx_bubbles_tsv) on the hand table of
// tests/bubbles_units.py, on random link tables (the twin's totals against a count of the lane function's classes, the identity of the totals, every row inside the
// table), and on tables that break the preconditions — a link to a segment past n_segs, offsets that fall, offsets past n_links, in-degrees of zero — which must be
// refused, not read: the arrays are sized exactly, so a read past them is the sanitizer's to report.  Exit status 0: every answer as expected (and the sanitizers silent).
// From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -o bubbles_san tests/tools/bubbles_san.cpp aligngraph_amd/csrc/agx_gfa.cpp && ./bubbles_san
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "../../aligngraph_amd/csrc/agx_host.h"
#include "../../include/agx.h"
namespace agx { unsigned usable_cpus() { return 1; } }      // (agx_gfa.cpp asks; its definition lives in agx_host.cpp, which this program does not link)

namespace {

int bad = 0;
void expect(bool ok, const char *what) { if (!ok) { printf("FAILED: %s\n", what); bad = 1; } }

// a unitig table over exactly sized arrays
struct Table {
    std::vector<uint32_t> hp, hv, nn, lp, lf, lt, sup; std::vector<uint64_t> cov, so; std::string seq; agx_unitigs t;
    Table(const std::vector<uint32_t> &nodes, const std::vector<std::pair<uint32_t, uint32_t> > &links) {
        const uint32_t n = (uint32_t)nodes.size();
        so.push_back(0);
        for (uint32_t s = 0; s < n; s++) {
            hp.push_back(100 * s); hv.push_back(s % 2); nn.push_back(nodes[s]); lp.push_back(100 * s + nodes[s] - 1); cov.push_back(10 * s + 1);
            for (uint32_t j = 0; j < nodes[s]; j++) seq += "ACGT"[(s + j) % 4];
            so.push_back(seq.size());
        }
        for (size_t i = 0; i < links.size(); i++) { lf.push_back(links[i].first); lt.push_back(links[i].second); sup.push_back(1000 + (uint32_t)i); }
        view();
    }
    void view() {
        memset(&t, 0, sizeof t);
        t.n_segs = (uint32_t)hp.size(); t.n_links = (uint32_t)lf.size(); t.n_bases = seq.size();
        t.head_pos = hp.data(); t.head_var = hv.data(); t.n_nodes = nn.data(); t.last_pos = lp.data(); t.coverage = cov.data(); t.seq_off = so.data(); t.seq = &seq[0];
        t.link_from = lf.data(); t.link_to = lt.data();
    }
};

// offsets, in-degrees and the classes by the lane function alone
struct Lanes {
    std::vector<uint32_t> l_off, s_in; uint64_t n[7] = {0, 0, 0, 0, 0, 0, 0};
    explicit Lanes(const Table &T) : l_off(T.hp.size() + 1, 0), s_in(T.hp.size(), 0) {
        const uint32_t ns = (uint32_t)T.hp.size(), nl = (uint32_t)T.lf.size();
        for (uint32_t i = 0; i < nl; i++) { l_off[T.lf[i] + 1]++; s_in[T.lt[i]]++; }
        for (uint32_t s = 0; s < ns; s++) l_off[s + 1] += l_off[s];
        for (uint32_t s = 0; s < ns; s++) n[agx_bubble_class(s, l_off.data(), T.lt.data(), s_in.data(), T.nn.data(), ns, nl).cls]++;
    }
};

void check_rows(const agx_bubbles &b, const Table &T, const char *what) {
    expect(b.n_forks == b.n_bubbles_all + b.n_tip + b.n_nested + b.n_sinks_differ + b.n_sink_shared, what);
    expect(b.br_off[0] == 0 && b.br_off[b.n_bubbles] == b.n_branches && b.br_seq_off[b.n_branches] == b.n_bases && b.n_bases <= T.seq.size() && b.n_branches <= T.lf.size(), what);
    for (uint32_t i = 0; i < b.n_bubbles; i++) expect(b.br_off[i + 1] >= b.br_off[i] + 2, what);
    for (uint32_t r = 0; r < b.n_branches; r++) expect(b.br_seq_off[r + 1] - b.br_seq_off[r] == b.br_nodes[r] && b.br_nodes[r] <= b.max_nodes, what);
}

}  // namespace

int main() {
    // the hand table of tests/bubbles_units.py
    const std::vector<std::pair<uint32_t, uint32_t> > links = {{0, 1}, {0, 2}, {0, 3}, {1, 3}, {2, 3}, {3, 4}, {3, 5}, {4, 6}, {5, 6}, {7, 8}, {7, 9}, {9, 10}, {11, 12}, {11, 13}, {12, 14}, {12, 15},
                                                               {13, 15}, {16, 17}, {16, 18}, {17, 19}, {18, 20}, {21, 22}, {21, 23}, {22, 24}, {23, 24}, {25, 24}};
    const std::vector<uint32_t> nodes = {3, 2, 5, 4, 1, 1, 2, 1, 2, 3, 1, 2, 1, 3, 1, 2, 2, 1, 1, 3, 1, 2, 2, 2, 1, 4};
    Table H(nodes, links);
    {
        Lanes L(H);
        expect(L.n[AGX_BB_BUBBLE] == 2 && L.n[AGX_BB_TIP] == 2 && L.n[AGX_BB_NESTED] == 1 && L.n[AGX_BB_SINKS_DIFFER] == 1 && L.n[AGX_BB_SINK_SHARED] == 1 && L.n[AGX_BB_BAD] == 0, "hand table: classes");
        const agx_bubble b0 = agx_bubble_class(0, L.l_off.data(), H.lt.data(), L.s_in.data(), H.nn.data(), 26, 26);
        expect(b0.cls == AGX_BB_BUBBLE && b0.sink == 3 && b0.k == 3 && b0.longest == 5 && b0.bases == 7, "hand table: the three-way bubble");
        for (uint32_t mx : {0xFFFFFFFFu, 6u, 5u, 4u, 0u}) for (int with : {0, 1}) {
            agx_bubbles b;
            expect(agx_unitigs_bubbles(&H.t, with ? H.sup.data() : nullptr, mx, &b) == AGX_OK, "hand table: the twin");
            expect(b.n_forks == 7 && b.n_bubbles_all == 2 && b.longest_branch == 5 && b.n_bubbles == (mx >= 5 ? 2u : mx >= 1 ? 1u : 0u), "hand table: totals and max_nodes");
            check_rows(b, H, "hand table: rows");
            char *text = nullptr; size_t len = 0;
            expect(agx_bubbles_tsv(&b, 7, &text, &len) == AGX_OK && (len == 0) == (b.n_bubbles == 0), "hand table: text");
            if (mx == 5 && with) {
                printf("%s", text);
                expect(std::string(text, len).find("u7_0_0\tu7_300_1\t2\t300\t3\tu7_100_1,u7_200_0,*\t2,5,0\t11,21,0\t1000,1001,1002\t1003,1004,1002\tCG,GTACG,*\n") == 0, "hand table: the first line");
            }
            agx_text_free(text);
            agx_bubbles_free(&b);
        }
    }
    // random forward link tables: the twin's totals are a count of the lane function's classes
    srand(18);
    uint64_t forks = 0, bubbles = 0;
    for (int round = 0; round < 400; round++) {
        const uint32_t ns = 1 + rand() % 40;
        std::vector<uint32_t> nn(ns);
        for (auto &v : nn) v = 1 + rand() % 6;
        std::vector<std::pair<uint32_t, uint32_t> > ls;
        for (uint32_t a = 0; a + 1 < ns; a++) for (uint32_t b = a + 1; b < ns && b < a + 5; b++)      // even rounds: a strand with skips of one or two (deletions); odd ones: anything forward
            if (round % 2 ? rand() % 100 < 40 : b == a + 1 ? rand() % 100 < 95 : b < a + 4 && rand() % 100 < 15) ls.emplace_back(a, b);
        Table T(nn, ls);
        Lanes L(T);
        const uint32_t mx = round % 3 ? 0xFFFFFFFFu : (uint32_t)(rand() % 7);
        agx_bubbles b;
        expect(agx_unitigs_bubbles(&T.t, round % 2 ? T.sup.data() : nullptr, mx, &b) == AGX_OK, "random table: the twin");
        expect(L.n[AGX_BB_BAD] == 0 && b.n_bubbles_all == L.n[AGX_BB_BUBBLE] && b.n_tip == L.n[AGX_BB_TIP] && b.n_nested == L.n[AGX_BB_NESTED] && b.n_sinks_differ == L.n[AGX_BB_SINKS_DIFFER] &&
               b.n_sink_shared == L.n[AGX_BB_SINK_SHARED], "random table: totals");
        check_rows(b, T, "random table: rows");
        char *text = nullptr; size_t len = 0;
        expect(agx_bubbles_tsv(&b, 0, &text, &len) == AGX_OK, "random table: text");
        agx_text_free(text);
        forks += b.n_forks; bubbles += b.n_bubbles_all;
        agx_bubbles_free(&b);
    }
    printf("random tables: %llu forks, %llu bubbles\n", (unsigned long long)forks, (unsigned long long)bubbles);
    expect(forks > 1000 && bubbles > 100, "random tables reach forks and bubbles");
    // broken tables: the twin refuses them, the lane function says BAD without reading behind the offending index
    {
        agx_bubbles b;
        Table T(nodes, links); T.lt[4] = 26; T.view();
        expect(agx_unitigs_bubbles(&T.t, T.sup.data(), 0xFFFFFFFFu, &b) == AGX_E_ARG, "a link to a segment past n_segs");
        Table U(nodes, links); U.lf[5] = 0; U.view();
        expect(agx_unitigs_bubbles(&U.t, nullptr, 0xFFFFFFFFu, &b) == AGX_E_ARG, "links not ordered by source");
        Table V(nodes, links); V.lf[3] = 26; V.view();
        expect(agx_unitigs_bubbles(&V.t, nullptr, 0xFFFFFFFFu, &b) == AGX_E_ARG, "a link from a segment past n_segs");
        Table W(nodes, links); W.so[3] += 1; W.view();
        expect(agx_unitigs_bubbles(&W.t, nullptr, 0xFFFFFFFFu, &b) == AGX_E_ARG, "bases that are not the nodes");
        expect(agx_unitigs_bubbles(nullptr, nullptr, 0, &b) == AGX_E_ARG && agx_unitigs_bubbles(&H.t, nullptr, 0, nullptr) == AGX_E_ARG, "null arguments");
        Lanes L(H);
        auto cls = [&](const std::vector<uint32_t> &off, const std::vector<uint32_t> &to, const std::vector<uint32_t> &in, uint32_t s) {
            return agx_bubble_class(s, off.data(), to.data(), in.data(), H.nn.data(), 26, (uint32_t)to.size()).cls; };
        std::vector<uint32_t> off = L.l_off, to = H.lt, in = L.s_in;
        expect(cls(off, to, in, 26) == AGX_BB_BAD && cls(off, to, in, 0xFFFFFFFFu) == AGX_BB_BAD, "a segment past n_segs");
        off[1] = 30;                                            // past n_links
        expect(cls(off, to, in, 0) == AGX_BB_BAD, "offsets past n_links");
        off = L.l_off; off[1] = 2; off[2] = 1;                  // offsets that fall (segment 1), seen from its fork (segment 0) and from itself
        expect(cls(off, to, in, 1) == AGX_BB_BAD && cls(off, to, in, 0) == AGX_BB_BAD, "offsets that fall");
        off = L.l_off; to[1] = 4000000000u;
        expect(cls(off, to, in, 0) == AGX_BB_BAD, "a target past n_segs");
        to = H.lt; to[3] = 77;                                  // the link out of branch segment 1
        expect(cls(off, to, in, 0) == AGX_BB_BAD, "a branch segment's exit past n_segs");
        to = H.lt; in[2] = 0;
        expect(cls(off, to, in, 0) == AGX_BB_BAD, "a target nothing enters");
        in = L.s_in; in[3] = 2;                                 // fewer links enter the sink than leave the source
        expect(cls(off, to, in, 0) == AGX_BB_BAD, "a sink with fewer links than branches");
    }
    // text of tables that do not describe themselves
    {
        agx_bubbles b; char *text = nullptr; size_t len = 0;
        expect(agx_unitigs_bubbles(&H.t, H.sup.data(), 0xFFFFFFFFu, &b) == AGX_OK, "the twin");
        b.br_off[1] = 6;
        expect(agx_bubbles_tsv(&b, 0, &text, &len) == AGX_E_ARG && !text, "branch offsets past the rows");
        b.br_off[1] = 3; b.br_seq_off[5] = 10;
        expect(agx_bubbles_tsv(&b, 0, &text, &len) == AGX_E_ARG && !text, "base offsets past the bases");
        b.br_seq_off[5] = 9;
        expect(agx_bubbles_tsv(&b, 0, &text, &len) == AGX_OK, "the table again");
        agx_text_free(text);
        expect(agx_bubbles_tsv(&b, -1, &text, &len) == AGX_E_ARG, "a negative unit");
        agx_bubbles_free(&b);
    }
    printf(bad ? "bubbles_san: FAILED\n" : "bubbles_san: ok\n");
    return bad;
}
