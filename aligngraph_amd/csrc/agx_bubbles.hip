// agx_bubbles.hip — gfx950 kernels of the bubbles (agx_unit_bubbles).
//
// They run behind phase 3 of a region export, on its stream, over the segment and link tables it left in the export's scratch, and decide every fork of that graph
// (agx_bubble_class, agx_core.h): a pass over the links for the in-degrees, a pass over the segments for the classes, three scans (the multi-launch scan) that place the
// bubbles, their branch rows and their bases, and the passes that write the table.  The kernels read the export's tables and write only the call's own arrays; every
// index is held against the count of what it names before anything is read or stored there, every loop runs to a count it read, and no atomic's return value is used.
#include <hip/hip_runtime.h>
#include "agx_kargs.h"

namespace {

__device__ __forceinline__ agx_u32 bb_sum32(agx_u32 v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ agx_u32 bb_max32(agx_u32 v) {
    for (int d = 32; d > 0; d >>= 1) { const agx_u32 o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// a thread per link: one more enters its target
__global__ void __launch_bounds__(256) agx_k_bb_indeg(agx_bubbles_args A) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_links) return;
    const agx_u32 t = A.l_to[i];
    if (t < A.n_segs) atomicAdd(A.s_in + t, 1u); else atomicOr(A.err, 16u);
}

// A thread per segment and one more for the closing zeros: the class, the flag after max_nodes, the rows and bases a flagged bubble takes.  A wavefront leaves its
// counts as one partial.  The totals count every fork whatever max_nodes.
__global__ void __launch_bounds__(256) agx_k_bb_class(agx_bubbles_args A) {
    const agx_u32 s = blockIdx.x * 256u + threadIdx.x, wave = s >> 6, lane = threadIdx.x & 63u;
    agx_bubble b{AGX_BB_NONE, AGX_NONE, 0u, 0u, 0u};
    if (s < A.n_segs) b = agx_bubble_class(s, A.l_off, A.l_to, A.s_in, A.s_len, A.n_segs, A.n_links);
    const bool bubble = b.cls == AGX_BB_BUBBLE, flagged = bubble && b.longest <= A.max_nodes;
    if (s <= A.n_segs) { A.flag[s] = flagged ? 1u : 0u; A.kcnt[s] = flagged ? b.k : 0u; A.bcnt[s] = flagged ? b.bases : 0u; }
    const agx_u32 n_fork = bb_sum32(b.cls != AGX_BB_NONE && b.cls != AGX_BB_BAD ? 1u : 0u), n_bub = bb_sum32(bubble ? 1u : 0u), n_tip = bb_sum32(b.cls == AGX_BB_TIP ? 1u : 0u),
                  n_nest = bb_sum32(b.cls == AGX_BB_NESTED ? 1u : 0u), n_diff = bb_sum32(b.cls == AGX_BB_SINKS_DIFFER ? 1u : 0u), n_shared = bb_sum32(b.cls == AGX_BB_SINK_SHARED ? 1u : 0u),
                  longest = bb_max32(bubble ? b.longest : 0u), n_bad = bb_sum32(b.cls == AGX_BB_BAD ? 1u : 0u);
    if (lane == 0 && wave < A.n_part) {
        agx_u32 *p = A.part + 8u * (size_t)wave;
        p[0] = n_fork; p[1] = n_bub; p[2] = n_tip; p[3] = n_nest; p[4] = n_diff; p[5] = n_shared; p[6] = longest; p[7] = n_bad;
    }
}

// one wavefront sums the partials (a unit's segments are counted in 32 bits, so are these)
__global__ void __launch_bounds__(64) agx_k_bb_totals(agx_bubbles_args A) {
    const agx_u32 lane = threadIdx.x;
    agx_u32 v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (agx_u32 w = lane; w < A.n_part; w += 64u) {
        const agx_u32 *p = A.part + 8u * (size_t)w;
        for (int j = 0; j < 8; j++) v[j] = j == 6 ? (p[j] > v[j] ? p[j] : v[j]) : v[j] + p[j];
    }
    for (int j = 0; j < 8; j++) v[j] = j == 6 ? bb_max32(v[j]) : bb_sum32(v[j]);
    if (lane == 0) for (int j = 0; j < 8; j++) A.tot[j] = v[j];
}

// A thread per flagged segment: the bubble's row at the place the flags' scan gives it, and its k branch rows in the order of its links.  The fork is classed again (the
// sink is not kept per segment); a branch row's two link numbers go where agx_k_bb_support puts their support.
__global__ void __launch_bounds__(256) agx_k_bb_emit(agx_bubbles_args A) {
    const agx_u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s >= A.n_segs || !A.flag[s]) return;
    const agx_bubble b = agx_bubble_class(s, A.l_off, A.l_to, A.s_in, A.s_len, A.n_segs, A.n_links);
    const agx_u32 at = A.boff[s], r0 = A.koff[s];
    agx_u32 base = A.baoff[s];
    if (b.cls != AGX_BB_BUBBLE || b.sink >= A.n_segs || at >= A.bub_cap || r0 > A.row_cap || b.k > A.row_cap - r0) { atomicOr(A.err, 16u); return; }
    A.b_spos[at] = A.s_hpos[s]; A.b_svar[at] = A.s_hvar[s]; A.b_slast[at] = A.s_last[s]; A.b_tpos[at] = A.s_hpos[b.sink]; A.b_tvar[at] = A.s_hvar[b.sink]; A.b_broff[at] = r0;
    const agx_u32 lo = A.l_off[s];
    for (agx_u32 j = 0; j < b.k; j++) {
        const agx_u32 i = lo + j, x = A.l_to[i], r = r0 + j;      // (lo + k <= n_links and every target < n_segs: the class just read them)
        if (A.s_in[x] == 1u) {
            const agx_u32 n = A.s_len[x];
            A.r_pos[r] = A.s_hpos[x]; A.r_var[r] = A.s_hvar[x]; A.r_nodes[r] = n; A.r_cov[r] = A.s_cov[x]; A.r_seqoff[r] = base; A.r_seg[r] = x; A.r_in[r] = i; A.r_out[r] = A.l_off[x];
            base += n;
        } else {
            A.r_pos[r] = AGX_NONE; A.r_var[r] = AGX_NONE; A.r_nodes[r] = 0u; A.r_cov[r] = 0ull; A.r_seqoff[r] = base; A.r_seg[r] = AGX_NONE; A.r_in[r] = i; A.r_out[r] = i;
        }
    }
}

// a wavefront per branch row: the bases of its segment, lane after lane
__global__ void __launch_bounds__(256) agx_k_bb_bases(agx_bubbles_args A) {
    const agx_u32 r = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (r >= A.row_cap) return;
    const agx_u32 x = A.r_seg[r];
    if (x == AGX_NONE) return;
    if (x >= A.n_segs) { atomicOr(A.err, 16u); return; }
    const agx_u32 n = A.s_len[x], from = A.s_off[x], to = A.r_seqoff[r];
    if (from > A.n_bases || n > A.n_bases - from || to > A.base_cap || n > A.base_cap - to) { atomicOr(A.err, 16u); return; }
    for (agx_u32 i = lane; i < n; i += 64u) A.o_seq[to + i] = A.seq[from + i];
}

// a thread per branch row: the two link numbers become the links' support
__global__ void __launch_bounds__(256) agx_k_bb_support(agx_bubbles_args A) {
    const agx_u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= A.row_cap) return;
    const agx_u32 i = A.r_in[r], o = A.r_out[r];
    if (i >= A.n_links || o >= A.n_links) { atomicOr(A.err, 16u); return; }
    A.r_in[r] = A.l_sup[i]; A.r_out[r] = A.l_sup[o];
}

inline dim3 bb_grid(unsigned long long n) { return dim3((unsigned)((n + 255u) / 256u)); }

}  // namespace

extern "C" agx_u32 agx_bubbles_partials(agx_u32 n_segs) { return (agx_u32)(((unsigned long long)n_segs + 1u + 255u) / 256u) * 4u; }

extern "C" void agx_launch_bubbles_class(const agx_bubbles_args *A, hipStream_t st) {
    if (A->n_links) hipLaunchKernelGGL(agx_k_bb_indeg, bb_grid(A->n_links), dim3(256), 0, st, *A);
    hipLaunchKernelGGL(agx_k_bb_class, bb_grid((unsigned long long)A->n_segs + 1u), dim3(256), 0, st, *A);
    hipLaunchKernelGGL(agx_k_bb_totals, dim3(1), dim3(64), 0, st, *A);
    agx_launch_exclusive_scan(A->flag, A->boff, A->n_segs, A->scan_tmp, st);
    agx_launch_exclusive_scan(A->kcnt, A->koff, A->n_segs, A->scan_tmp, st);
    agx_launch_exclusive_scan(A->bcnt, A->baoff, A->n_segs, A->scan_tmp, st);
}

extern "C" void agx_launch_bubbles_emit(const agx_bubbles_args *A, hipStream_t st) {
    if (!A->bub_cap) return;
    hipLaunchKernelGGL(agx_k_bb_emit, bb_grid(A->n_segs), dim3(256), 0, st, *A);
    if (A->base_cap) hipLaunchKernelGGL(agx_k_bb_bases, bb_grid((unsigned long long)A->row_cap * 64u), dim3(256), 0, st, *A);
    if (A->l_sup) hipLaunchKernelGGL(agx_k_bb_support, bb_grid(A->row_cap), dim3(256), 0, st, *A);
}
