// links_san.cpp — a stand-alone program for a sanitizer run of the host-side pieces of the mate links on the CPU: the probe loop
// (agx_links_insert) and the range-halving planner (agx::links_plan) through the serial replay of tests/links_shim.cpp on a hand-made unit of four records at 2 (refused), 4
// (split), 8 and 64 slots, and the TSV formatter (agx_mate_links_tsv).  Exit status 0: every answer as expected (and the sanitizers silent).  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -o links_san tests/tools/links_san.cpp tests/links_shim.cpp \
//       aligngraph_amd/csrc/agx_gfa.cpp && ./links_san
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../aligngraph_amd/csrc/agx_host.h"
#include "../../include/agx.h"
namespace agx { unsigned usable_cpus() { return 1; } }      // (agx_gfa.cpp asks; its definition lives in agx_host.cpp, which this program does not link)
extern "C" int agx_links_shim(const agx_dhit *, uint32_t, const agx_run *, uint32_t, uint32_t, const uint32_t *, uint32_t, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                              const uint8_t *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t *, uint32_t *, uint32_t *, uint64_t *, uint64_t *, uint32_t *, uint32_t);
int main() {
    const uint32_t n_pos = 40;
    struct H { uint32_t a, b, len, skip; } hs[] = {{2, 10, 2, 0}, {3, 20, 2, 0}, {2, 30, 2, 0}, {12, 31, 2, 0}, {21, 4, 1, 1}, {11, 22, 3, 0}, {36, 38, 6, 0}};
    std::vector<agx_dhit> d(7); memset(d.data(), 0, 7 * sizeof(agx_dhit));
    for (int i = 0; i < 7; i++) { d[i].a_t0 = hs[i].a; d[i].b_t0 = hs[i].b; d[i].len = hs[i].len; d[i].flags = hs[i].skip ? AGX_HF_SKIP : 0; }
    agx_run run0; memset(&run0, 0, sizeof run0);
    uint32_t st_first[4] = {0, 10, 20, 30}, st_base[4] = {0, 0, 0, 0}, st_rec[4] = {0, 1, 2, 3}, st_pre[5] = {0, 6, 12, 18, 24}; uint8_t st_join[5] = {0, 0, 0, 0, 0};
    uint32_t side[1] = {0};
    int bad = 0;
    for (uint32_t slots : {2u, 4u, 8u, 64u}) for (uint32_t mp : {0u, 1u, 2u}) {
        uint64_t totals[13]; std::vector<uint32_t> rec(20), own(n_pos), num(5 * 7); std::vector<uint64_t> key(7), len(7);
        const int rc = agx_links_shim(d.data(), 7, &run0, 1, n_pos, side, n_pos, st_first, st_base, st_rec, st_pre, st_join, 4, 24, 4, mp, slots, totals, rec.data(), own.data(), key.data(), len.data(), num.data(), 7);
        printf("slots %u min_pairs %u: rc %d, passes %llu, links %llu, distinct %llu\n", slots, mp, rc, (unsigned long long)totals[9], (unsigned long long)totals[10], (unsigned long long)totals[8]);
        if (slots == 2 ? rc != -1 : (rc != 0 || totals[8] != 5)) bad = 1;
    }
    uint32_t a[2] = {0, 1}, b[2] = {1, 0}, n[2] = {2, 1}, lo[2] = {12, 3}; uint64_t ls[2] = {24, 9};
    agx_mate_links l; memset(&l, 0, sizeof l);
    l.n_recs = 2; l.n_links = 2; l.a = a; l.b = b; l.n_pairs = n; l.len_sum = ls; l.lo_min = lo; l.lo_max = lo; l.hi_min = lo; l.hi_max = lo;
    char *text = nullptr; size_t tl = 0;
    const int rc = agx_mate_links_tsv(&l, 3, &text, &tl);
    printf("tsv rc %d, %zu bytes:\n%s", rc, tl, text ? text : "");
    if (rc != 0) bad = 1;
    agx_text_free(text);
    return bad;
}
