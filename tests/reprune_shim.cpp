// reprune_shim.cpp — TEST-ONLY: agx_reprune_lane (csrc/agx_core.h) run serially, tile by tile, over plain arrays, the way agx_k_reprune runs it on the device
// (a wavefront per tile, lane = position): the in-tile prefix of the lanes' side counts is done in plain C here, by the DPP scan there.
// tests/test_reprune_lane.py compiles this into a shared library with g++ and compares its outputs with numpy.  With -DAGX_REPRUNE_SHIM_MAIN it is a program of its own
// (for a sanitizer build): made-up tables, every threshold of the test, checked against a second, naive count.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_core.h"

extern "C" int agx_reprune_shim(const uint32_t *node_start, const uint16_t *node_cnt, const uint32_t *nk_cid, const int *n_counts, uint8_t *n_flags,
                                uint32_t n_pos, uint32_t pool_cap, uint32_t coverage, uint32_t *side_pk, uint32_t *tile_side) {
    if (coverage > 0x7FFFFFFFu) return -1;
    agx_reprune_args A;
    A.node_start = node_start; A.node_cnt = node_cnt; A.nk_cid = nk_cid; A.n_counts = n_counts; A.n_flags = n_flags;
    A.side_pk = side_pk; A.tile_side = tile_side; A.n_pos = n_pos; A.pool_cap = pool_cap; A.coverage = (int)coverage; A.abort = nullptr;
    const uint32_t n_tiles = (n_pos + AGX_TILE - 1) / AGX_TILE;
    for (uint32_t tile = 0; tile < n_tiles; tile++) {
        uint32_t before = 0;
        for (uint32_t lane = 0; lane < AGX_TILE; lane++) {
            const uint32_t X = tile * AGX_TILE + lane;
            const uint32_t side = agx_reprune_lane(A, X);      // (0 past n_pos)
            if (X < n_pos) side_pk[X] = agx_side_pack(before, side);
            before += side;
        }
        tile_side[tile] = before;
    }
    return 0;
}

#ifdef AGX_REPRUNE_SHIM_MAIN
int main() {
    const uint32_t thresholds[] = {0u, 1u, 3u, 5u, 8u, 20u, 1u << 30};
    uint32_t x = 12345u; auto rnd = [&] { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    int bad = 0;
    for (uint32_t n_pos : {1u, 63u, 64u, 65u, 1000u, 4099u}) {
        std::vector<uint32_t> start(n_pos); std::vector<uint16_t> cnt(n_pos); uint32_t nodes = 0;
        for (uint32_t p = 0; p < n_pos; p++) {      // mostly one variant; holes; a pile of the widest positions at the end of a tile
            const uint32_t r = rnd() % 100u, n = (p % 64u >= 60u && p / 64u == 1u) ? AGX_MAXV_HUGE : r < 5u ? 0u : r < 90u ? 1u : 2u + rnd() % 6u;
            start[p] = nodes; cnt[p] = (uint16_t)n; nodes += n;
        }
        std::vector<uint32_t> cid(nodes); std::vector<int> counts((size_t)nodes * 6); std::vector<uint8_t> flags(nodes), flags0;
        for (uint32_t v = 0; v < nodes; v++) { cid[v] = rnd() % 4u ? AGX_NONE : rnd() % 7u; counts[(size_t)v * 6] = (int)(rnd() % 30u); flags[v] = (uint8_t)(rnd() & 0xFFu); }
        flags0 = flags;
        const uint32_t n_tiles = (n_pos + 63u) / 64u;
        std::vector<uint32_t> pk(n_pos), ts(n_tiles);
        for (uint32_t c : thresholds) {
            if (agx_reprune_shim(start.data(), cnt.data(), cid.data(), counts.data(), flags.data(), n_pos, nodes, c, pk.data(), ts.data()) != 0) { bad++; continue; }
            unsigned long long sum = 0, want = 0;
            for (uint32_t p = 0; p < n_pos; p++) {
                uint32_t alive = 0;
                for (uint32_t v = start[p]; v < start[p] + cnt[p]; v++) {
                    const bool dead = cid[v] == AGX_NONE && counts[(size_t)v * 6] < (int)c;
                    if (((flags[v] & AGX_NF_DEAD) != 0) != dead || ((flags[v] ^ flags0[v]) & ~AGX_NF_DEAD)) bad++;
                    alive += dead ? 0u : 1u;
                }
                const uint32_t side = alive ? alive - 1 : 0;
                if ((pk[p] >> 16) != side) bad++;
                want += side;
            }
            for (uint32_t t = 0; t < n_tiles; t++) sum += ts[t];
            if (sum != want) bad++;
        }
    }
    printf("reprune shim: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
