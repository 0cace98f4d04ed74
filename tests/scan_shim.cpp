// scan_shim.cpp — TEST-ONLY: the look-back of the one-launch scan (agx_k_scan_lookback, agx_kernels.hip) replayed serially on the CPU over a descriptor array in any
// state.  What a lane takes from a window is agx_scan_window_take (csrc/agx_core.h), the function the kernel calls; the ballot, the sum over the lanes and the walk
// from window to window are plain loops here, wavefront instructions there.  tests/test_scan_cases.py compiles this into a shared library with g++ and compares it
// with tests/scan_model.py, which shares nothing with it.  With -DAGX_SCAN_SHIM_MAIN it is a program of its own (for a sanitizer build): descriptor arrays in random
// states, every block's look-back against a plain backward walk.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../aligngraph_amd/csrc/agx_core.h"

// One window: the predecessors hi, hi - 1, .., hi - 63 of desc[] (lanes in front of block 0 hold AGX_SCAN_FRONT).  parts[64]: what each lane takes; *last: the walk ends here.
// Returns 0, or -1 if a lane's descriptor is not published (the kernel would wait for it).
extern "C" int agx_scan_window_shim(const unsigned long long *desc, long long hi, uint32_t *parts, int *last) {
    unsigned long long d[64], pfx = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const long long j = hi - (long long)lane;
        d[lane] = j >= 0 ? desc[j] : AGX_SCAN_FRONT;
        if ((d[lane] >> 62) == 0) return -1;
        if (agx_scan_is_prefix(d[lane])) pfx |= 1ull << lane;
    }
    bool l = false;
    for (uint32_t lane = 0; lane < 64; lane++) { bool mine; parts[lane] = agx_scan_window_take(pfx, d[lane], lane, mine); if (lane == 0) l = mine; else if (mine != l) return -2; }      // (wave-uniform)
    *last = l ? 1 : 0;
    return 0;
}

// The whole look-back of block b, as the kernel's loop runs it: *excl = the block's exclusive prefix, *windows = the windows it read.
extern "C" int agx_scan_lookback_shim(const unsigned long long *desc, uint32_t b, uint32_t *excl, uint32_t *windows) {
    uint32_t e = 0, w = 0;
    for (long long hi = (long long)b - 1; hi >= 0;) {
        uint32_t parts[64]; int last = 0;
        const int rc = agx_scan_window_shim(desc, hi, parts, &last);
        if (rc) return rc;
        uint32_t part = 0;
        for (uint32_t lane = 0; lane < 64; lane++) part += parts[lane];
        e += part; w++;
        if (last) break;
        hi -= 64;
    }
    *excl = e; *windows = w;
    return 0;
}

#ifdef AGX_SCAN_SHIM_MAIN
int main() {
    uint32_t x = 2463534242u; auto rnd = [&] { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    int bad = 0;
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 66u, 128u, 129u, 130u, 301u}) {
        for (uint32_t density : {0u, 1u, 3u, 64u, 65u, 1000u}) {       // a prefix every `density` blocks or so; 0: every block; 1000: block 0 alone
            std::vector<unsigned long long> desc(n);
            std::vector<uint32_t> total(n), incl(n);
            uint32_t run = 0;
            for (uint32_t b = 0; b < n; b++) {
                total[b] = (rnd() & 1u) ? 0xFFFFFFFFu : rnd(); run += total[b]; incl[b] = run;
                const bool is_pfx = b == 0 || density == 0 || (density < 1000u && rnd() % density == 0);
                desc[b] = is_pfx ? (AGX_SCAN_PFX | incl[b]) : (AGX_SCAN_AGG | total[b]);
            }
            for (uint32_t b = 0; b <= n; b++) {
                uint32_t excl = 0, windows = 0;
                if (agx_scan_lookback_shim(desc.data(), b, &excl, &windows) != 0) { bad++; continue; }
                uint32_t want = 0, steps = 0; bool met = false;
                for (long long j = (long long)b - 1; j >= 0 && !met; j--) { want += (uint32_t)desc[j]; steps++; met = (desc[j] >> 62) == 2; }
                const uint32_t want_windows = b == 0 ? 0u : (steps + 63u) / 64u;
                if (excl != want || excl != (b ? incl[b - 1] : 0u) || windows != want_windows) bad++;
            }
        }
    }
    printf("scan shim: %s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif
