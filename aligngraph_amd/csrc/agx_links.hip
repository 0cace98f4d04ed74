// agx_links.hip — gfx950 kernels of the mate links (agx_unit_mate_links).
//
// own[x] is the smallest record with a graph base on position x (agx_k_ln_own: an atomic minimum per flat base of §14's table).  A kept hit's fragment [f_lo, f_hi]
// (agx_span_fragment, §16) is classed by own[f_lo] and own[f_hi] (agx_links_class); a fragment whose ends lie under two different records is a pair of the LINK
// (A, B), A under the left end.  The links are aggregated by their 64-bit key into a hash table in the export's scratch: linear probing from a multiply-shift home slot
// (agx_links_insert, agx_core.h), the key claimed by a 64-bit compare-and-swap, the numbers by atomic add, minimum and maximum.  The minima are set by agx_k_ln_init and
// not by the lane that claims a slot: a lane that finds the key present may accumulate before any further store of the claimer would land.  The slots in use and at the
// caller's threshold are flagged, scanned (the multi-launch scan) and copied densely.  All arithmetic is integer and no atomic's return value decides anything but the
// slot, so the table's content is the same run to run, whatever slot a key lands in.  The kernels read the unit's arrays and write only the export's scratch; every index is
// held against the capacity of what it names before anything is read or stored there, and every loop runs to a count the kernel was given.
#include <hip/hip_runtime.h>
#include "agx_kargs.h"

namespace {

__device__ __forceinline__ agx_u32 ln_sum32(agx_u32 v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the fragment of hit record i, the record read as five 8-byte words (the fifth, x_lo / x_hi, is not needed): agx_span.hip's sp_fragment
__device__ __forceinline__ int ln_fragment(const agx_dhit *dhit, agx_u32 i, const agx_run *runs, agx_u32 n_runs, agx_u32 n_pos, agx_u32 *f_lo, agx_u32 *f_hi) {
    const uint2 *g = reinterpret_cast<const uint2 *>(dhit + i);
    const uint2 w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3];
    return agx_span_fragment_v(w0.x, w0.y, w1.x, w1.y, w2.y & 0xFFFFu, w3.x & 0xFFFFu, w3.x >> 16, w3.y, runs, n_runs, n_pos, f_lo, f_hi);
}

// own to none and the per-record counters to 0 (init_all), every slot empty: key all ones, both minima all ones, the rest 0.  A thread per entry of the longest array.
__global__ void __launch_bounds__(256) agx_k_ln_init(agx_links_args A) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (A.init_all) {
        if (i < A.n_pos) A.own[i] = AGX_NONE;
        if ((unsigned long long)i < 5ull * A.n_recs) A.rec[i] = 0u;
    }
    if (i < A.slots) {
        A.t_key[i] = AGX_LINKS_EMPTY; A.t_len[i] = 0ull; A.t_n[i] = 0u;
        A.t_lo_min[i] = AGX_NONE; A.t_lo_max[i] = 0u; A.t_hi_min[i] = AGX_NONE; A.t_hi_max[i] = 0u;
    }
}

// a thread per flat graph base: its record bids for its position
__global__ void __launch_bounds__(256) agx_k_ln_own(agx_links_args A) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.T.n_flat) return;
    const agx_evidence_base b = agx_evidence_lane(A.T, i);
    if (b.st == AGX_NONE || b.rec >= A.n_recs) return;
    const agx_u32 x = agx_span_pos(b.id, A.n_pos, A.T.n_ids, A.side_xpos);
    if (x < A.n_pos) atomicMin(A.own + x, b.rec);
}

// The shadow count: the lanes stride over the flat bases and the positions together — item i is flat base i (shadowed: its position's owner is another record) and
// position i (owned).  A wavefront leaves its two counts as one partial; the host sums them.
__global__ void __launch_bounds__(256) agx_k_ln_shadow(agx_links_args A) {
    const agx_u32 stride = gridDim.x * 256u, wave = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    const agx_u32 n = A.T.n_flat > A.n_pos ? A.T.n_flat : A.n_pos;
    agx_u32 n_shadowed = 0, n_owned = 0;
    for (agx_u32 base = blockIdx.x * 256u; base < n; base += stride) {
        const agx_u32 i = base + threadIdx.x;
        if (i < A.T.n_flat) {
            const agx_evidence_base b = agx_evidence_lane(A.T, i);
            if (b.st != AGX_NONE && b.rec < A.n_recs) {
                const agx_u32 x = agx_span_pos(b.id, A.n_pos, A.T.n_ids, A.side_xpos);
                if (x < A.n_pos && A.own[x] != b.rec) n_shadowed++;
            }
        }
        if (i < A.n_pos && A.own[i] != AGX_NONE) n_owned++;
        if (stride > 0xFFFFFFFFu - base) break;      // (the next base would wrap)
    }
    n_shadowed = ln_sum32(n_shadowed); n_owned = ln_sum32(n_owned);
    if (lane == 0 && wave < A.n_spart) { A.spart[2u * wave] = n_shadowed; A.spart[2u * wave + 1u] = n_owned; }
}

// The pass: the lanes stride over all hit records (agx_k_span_mark's loop).  count != 0: the per-record counters and the wavefront's partial of the totals.  A link whose
// left record lies in [a_lo, a_hi) goes into the table; a lane that runs out of probes adds 1 to the overflow word and drops its pair (the host discards the pass).
__global__ void __launch_bounds__(256) agx_k_ln_pass(agx_links_args A) {
    const agx_u32 stride = gridDim.x * 256u, wave = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    agx_u32 n_kept = 0, n_out = 0, n_unowned = 0, n_inside = 0, n_open = 0, n_link = 0;
    for (agx_u32 base = blockIdx.x * 256u; base < A.n_hits; base += stride) {      // (wave-uniform: the wavefront's lanes leave the loop together)
        const agx_u32 i = base + threadIdx.x;
        agx_u32 f_lo = 0, f_hi = 0; unsigned long long key = AGX_LINKS_EMPTY;      // key: the link this lane inserts, or none
        if (i < A.n_hits) {
            const int kind = ln_fragment(A.dhit, i, A.runs, A.n_runs, A.n_pos, &f_lo, &f_hi);
            n_kept += kind != AGX_SPAN_SKIPPED ? 1u : 0u;
            n_out += kind == AGX_SPAN_OUTSIDE ? 1u : 0u;
            if (kind == AGX_SPAN_FRAGMENT) {
                const agx_u32 a = f_lo < A.n_pos ? A.own[f_lo] : AGX_NONE, b = f_hi < A.n_pos ? A.own[f_hi] : AGX_NONE;
                const int cls = agx_links_class(a, b);
                if ((a != AGX_NONE && a >= A.n_recs) || (b != AGX_NONE && b >= A.n_recs)) atomicOr(A.words, 1u);      // (own holds what agx_k_ln_own put there: never)
                else {
                    if (A.count) {
                        if (cls == AGX_LINKS_UNOWNED) n_unowned++;
                        else if (cls == AGX_LINKS_INSIDE) { n_inside++; atomicAdd(A.rec + a, 1u); }
                        else if (cls == AGX_LINKS_OPEN_LEFT) { n_open++; atomicAdd(A.rec + (size_t)A.n_recs + b, 1u); }
                        else if (cls == AGX_LINKS_OPEN_RIGHT) { n_open++; atomicAdd(A.rec + 2 * (size_t)A.n_recs + a, 1u); }
                        else { n_link++; atomicAdd(A.rec + 3 * (size_t)A.n_recs + a, 1u); atomicAdd(A.rec + 4 * (size_t)A.n_recs + b, 1u); }
                    }
                    if (cls == AGX_LINKS_LINK && a >= A.a_lo && a < A.a_hi) key = agx_links_key(a, b);
                }
            }
        }
        if (key != AGX_LINKS_EMPTY)
            agx_links_insert(key, A.slots, A.log2_slots,
                [&](agx_u32 s, unsigned long long k) { return (unsigned long long)atomicCAS(A.t_key + s, AGX_LINKS_EMPTY, k); },
                [&](agx_u32 s) {
                    atomicAdd(A.t_n + s, 1u); atomicAdd(A.t_len + s, (unsigned long long)(f_hi - f_lo) + 1ull);
                    atomicMin(A.t_lo_min + s, f_lo); atomicMax(A.t_lo_max + s, f_lo); atomicMin(A.t_hi_min + s, f_hi); atomicMax(A.t_hi_max + s, f_hi);
                },
                [&]() { atomicAdd(A.words + 1, 1u); });
        if (stride > 0xFFFFFFFFu - base) break;      // (the next base would wrap)
    }
    if (!A.count) return;
    n_kept = ln_sum32(n_kept); n_out = ln_sum32(n_out); n_unowned = ln_sum32(n_unowned); n_inside = ln_sum32(n_inside); n_open = ln_sum32(n_open); n_link = ln_sum32(n_link);
    if (lane == 0 && wave < A.n_part) {
        agx_u32 *p = A.part + 6u * (size_t)wave;
        p[0] = n_kept; p[1] = n_out; p[2] = n_unowned; p[3] = n_inside; p[4] = n_open; p[5] = n_link;
    }
}

// The kept slots' flags: in use and at the threshold; the slots in use are counted whatever the threshold.  A thread per slot and one more for the flags' closing zero.
__global__ void __launch_bounds__(256) agx_k_ln_flag(agx_links_args A) {
    const agx_u32 s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool used = s < A.slots && A.t_key[s] != AGX_LINKS_EMPTY;
    if (s <= A.slots) A.flag[s] = used && A.t_n[s] >= A.min_pairs ? 1u : 0u;
    const agx_u32 n_used = (agx_u32)__popcll(__ballot(used));
    if (lane == 0 && n_used) atomicAdd(A.words + 2, n_used);
}

// a kept slot goes to the place the flags' scan gives it
__global__ void __launch_bounds__(256) agx_k_ln_emit(agx_links_args A) {
    const agx_u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s >= A.slots || !A.flag[s]) return;
    const agx_u32 at = A.off[s];
    if (at >= A.out_cap) { atomicOr(A.words, 2u); return; }
    A.o_key[at] = A.t_key[s]; A.o_len[at] = A.t_len[s]; A.o_n[at] = A.t_n[s];
    A.o_lo_min[at] = A.t_lo_min[s]; A.o_lo_max[at] = A.t_lo_max[s]; A.o_hi_min[at] = A.t_hi_min[s]; A.o_hi_max[at] = A.t_hi_max[s];
}

inline dim3 ln_grid(agx_u32 n) { return dim3((unsigned)(((unsigned long long)n + 255u) / 256u)); }
inline agx_u32 ln_blocks(agx_u32 n) { const agx_u32 b = (agx_u32)(((unsigned long long)n + 255u) / 256u); return b < 1u ? 1u : b > AGX_SPAN_BLOCKS ? AGX_SPAN_BLOCKS : b; }

}  // namespace

extern "C" agx_u32 agx_links_partials(agx_u32 n) { return ln_blocks(n) * 4u; }

extern "C" void agx_launch_links_init(const agx_links_args *A, hipStream_t st) {
    unsigned long long n = A->slots;
    if (A->init_all) { n = n > A->n_pos ? n : A->n_pos; n = n > 5ull * A->n_recs ? n : 5ull * A->n_recs; }
    hipLaunchKernelGGL(agx_k_ln_init, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, st, *A);
}

extern "C" void agx_launch_links_own(const agx_links_args *A, hipStream_t st) {
    if (A->T.n_flat) hipLaunchKernelGGL(agx_k_ln_own, ln_grid(A->T.n_flat), dim3(256), 0, st, *A);
    hipLaunchKernelGGL(agx_k_ln_shadow, dim3(ln_blocks(A->T.n_flat > A->n_pos ? A->T.n_flat : A->n_pos)), dim3(256), 0, st, *A);
}

extern "C" void agx_launch_links_pass(const agx_links_args *A, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_ln_pass, dim3(ln_blocks(A->n_hits)), dim3(256), 0, st, *A);
    hipLaunchKernelGGL(agx_k_ln_flag, ln_grid(A->slots + 1u), dim3(256), 0, st, *A);
    agx_launch_exclusive_scan(A->flag, A->off, A->slots, A->scan_tmp, st);
    hipLaunchKernelGGL(agx_k_ln_emit, ln_grid(A->slots), dim3(256), 0, st, *A);
}
