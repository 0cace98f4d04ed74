// agx_evidence.hip — gfx950 kernels of the evidence under the walk's records (agx_unit_walk_evidence).
//
// A graph base of a pre-extended record is a walk id; the id's node carries the coverage and the votes, the edge to the next base's node the events counted for it (§13).
// All of that is resident after a build: the join is one gather per base.  The bases of all stretches of the table, in the table's order, are numbered flat; a wavefront
// takes 64 consecutive flat bases, a lane finds its stretch by bisecting the prefix of the stretch lengths (agx_evidence_lane, agx_core.h) and reads a_nid, n_counts and,
// for its step, n_next / e_cnt (the overflow list for sources with AGX_NF_EOVF).  Weak intervals take the id map's shape (agx_k_idm_flags / agx_k_idm_runs): start flags,
// the multi-launch scan, then a runs kernel.  The kernels read the unit's arrays and write only the export's scratch; every index is held against the capacity of what it
// names before anything is read or stored there, and every loop runs to a count the kernel read.
#include <hip/hip_runtime.h>
#include "agx_kargs.h"

namespace {

constexpr unsigned long long EV_NONE64 = ~0ull;

// what the interval kernels ask of a base: is it weak, and where does it lie
struct ev_mark { bool weak; agx_u32 rec, off; };

// flat base i with its step looked up by the lane itself (lane 0's predecessor; the gather takes the neighbour lane's slot where it can)
__device__ __forceinline__ ev_mark ev_mark_of(const agx_evidence_args &A, agx_u32 i) {
    const agx_evidence_base b = agx_evidence_lane(A.T, i);
    ev_mark m{false, b.rec, b.off};
    if (b.st == AGX_NONE) return m;
    agx_u32 step = AGX_NONE; bool noedge = false;
    if (b.has_step && b.slot != AGX_NONE) {
        const agx_u32 ns = agx_evidence_slot(A.T, b.next_id);
        if (ns != AGX_NONE) step = agx_evidence_step(A.T, b.slot, ns, &noedge);
    }
    m.weak = agx_evidence_weak(b.depth, step, A.min_depth, A.min_support);
    return m;
}

__device__ __forceinline__ unsigned long long ev_min64(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long ev_sum64(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ agx_u32 ev_min32(agx_u32 v) {
    for (int d = 32; d > 0; d >>= 1) { const agx_u32 o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}

// The gather: per base depth, votes and step; per record the sums and the minima; the interval-start flags.  A thread per flat base of the chunk and one more for the
// flags' closing zero.
__global__ void __launch_bounds__(256) agx_k_ev_gather(agx_evidence_args A) {
    const agx_u32 j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = j < A.n;
    agx_evidence_base b{AGX_NONE, AGX_NONE, 0u, AGX_NONE, AGX_NONE, AGX_NONE, AGX_NONE, AGX_NONE, false, false};
    if (in) b = agx_evidence_lane(A.T, A.lo + j);
    const bool valid = in && b.st != AGX_NONE;
    // the step: its target's slot is the neighbour lane's where the step stays inside the stretch and the neighbour is a lane of this wavefront and a base of this chunk
    const agx_u32 nb_slot = __shfl_down(b.slot, 1, 64);
    agx_u32 step = AGX_NONE; bool noedge = false;
    if (valid && b.has_step && b.slot != AGX_NONE) {
        const agx_u32 ns = b.inner && lane < 63u && j + 1u < A.n ? nb_slot : agx_evidence_slot(A.T, b.next_id);
        if (ns != AGX_NONE) step = agx_evidence_step(A.T, b.slot, ns, &noedge);
    }
    if (noedge) atomicAdd(A.noedge, 1u);
    if (valid) { A.c_depth[j] = b.depth; A.c_step[j] = step; if (A.c_votes) A.c_votes[j] = b.votes; }

    // interval starts: weak, and the base in front (in (record, offset) order: the flat base in front) is not a weak base of the same record at offset - 1.
    // The chunk's first base has nothing in front: an interval cut by the chunk's border is merged on the host
    const bool weak = valid && agx_evidence_weak(b.depth, step, A.min_depth, A.min_support);
    ev_mark p;
    p.weak = __shfl_up((int)weak, 1, 64) != 0; p.rec = __shfl_up(b.rec, 1, 64); p.off = __shfl_up(b.off, 1, 64);
    if (lane == 0) { p.weak = false; if (valid && j > 0) p = ev_mark_of(A, A.lo + j - 1u); }
    if (j <= A.n) A.flag[j] = weak && !(p.weak && p.rec == b.rec && p.off + 1u == b.off) ? 1u : 0u;

    // record summaries: where the wavefront's bases belong to one record, one reduction and one atomic per quantity from lane 0, else per-lane atomics
    const bool rec_ok = valid && b.rec < A.n_recs;
    const unsigned long long steps = rec_ok && step != AGX_NONE ? 1ull : 0ull, dsum = rec_ok && b.depth != AGX_NONE ? (unsigned long long)b.depth : 0ull;
    const unsigned long long dkey = rec_ok && b.depth != AGX_NONE ? ((unsigned long long)b.depth << 32) | b.off : EV_NONE64;
    const unsigned long long skey = rec_ok && step != AGX_NONE ? ((unsigned long long)step << 32) | b.off : EV_NONE64;
    const agx_u32 r0 = __shfl(b.rec, 0, 64);
    const bool first_ok = __shfl((int)rec_ok, 0, 64) != 0;
    if (first_ok && __all(!rec_ok || b.rec == r0)) {
        const unsigned long long ts = ev_sum64(steps), td = ev_sum64(dsum), md = ev_min64(dkey), ms = ev_min64(skey);
        if (lane == 0) {
            if (ts) atomicAdd(A.r_steps + r0, ts);
            if (td) atomicAdd(A.r_dsum + r0, td);
            if (md != EV_NONE64) atomicMin(A.r_dmin + r0, md);
            if (ms != EV_NONE64) atomicMin(A.r_smin + r0, ms);
        }
    } else if (rec_ok) {
        if (steps) atomicAdd(A.r_steps + b.rec, steps);
        if (dsum) atomicAdd(A.r_dsum + b.rec, dsum);
        if (dkey != EV_NONE64) atomicMin(A.r_dmin + b.rec, dkey);
        if (skey != EV_NONE64) atomicMin(A.r_smin + b.rec, skey);
    }
}

// The intervals of the chunk: record, first and last base offset, the smallest depth and the smallest numbered step.  A weak base lies in interval foff[j + 1] - 1 (the
// starts at or in front of it, less one).  Minima: one wave reduction and one atomic where the wavefront's 64 bases lie in one interval, else per-lane atomics.
__global__ void __launch_bounds__(256) agx_k_ev_runs(agx_evidence_args A) {
    const agx_u32 j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = j < A.n;
    ev_mark m{false, AGX_NONE, 0u};
    agx_u32 depth = AGX_NONE, step = AGX_NONE;
    if (in) {
        const agx_evidence_base b = agx_evidence_lane(A.T, A.lo + j);
        if (b.st != AGX_NONE) { depth = A.c_depth[j]; step = A.c_step[j]; m.rec = b.rec; m.off = b.off; m.weak = agx_evidence_weak(depth, step, A.min_depth, A.min_support); }
    }
    ev_mark s;
    s.weak = __shfl_down((int)m.weak, 1, 64) != 0; s.rec = __shfl_down(m.rec, 1, 64); s.off = __shfl_down(m.off, 1, 64);
    if (lane == 63u) {
        s.weak = false;
        if (m.weak && j + 1u < A.n) {
            const agx_evidence_base b = agx_evidence_lane(A.T, A.lo + j + 1u);
            if (b.st != AGX_NONE) { s.rec = b.rec; s.off = b.off; s.weak = agx_evidence_weak(A.c_depth[j + 1u], A.c_step[j + 1u], A.min_depth, A.min_support); }
        }
    }
    if (j + 1u >= A.n) s.weak = false;
    agx_u32 r = AGX_NONE;
    if (m.weak) {
        r = A.foff[j + 1u] - 1u;
        if (r >= A.iv_cap) { atomicOr(A.err, 1u); r = AGX_NONE; }
    }
    const bool on = r != AGX_NONE;
    if (on) {
        if (A.flag[j]) { A.iv_rec[r] = m.rec; A.iv_first[r] = m.off; }
        if (!(s.weak && s.rec == m.rec && s.off == m.off + 1u)) A.iv_last[r] = m.off;
    }
    const agx_u32 r0 = __shfl(r, 0, 64);
    if (r0 != AGX_NONE && __all(on && r == r0)) {
        const agx_u32 md = ev_min32(depth), ms = ev_min32(step);
        if (lane == 0) { if (md != AGX_NONE) atomicMin(A.iv_dmin + r0, md); if (ms != AGX_NONE) atomicMin(A.iv_smin + r0, ms); }
    } else if (on) {
        if (depth != AGX_NONE) atomicMin(A.iv_dmin + r, depth);
        if (step != AGX_NONE) atomicMin(A.iv_smin + r, step);
    }
}

inline dim3 ev_grid(agx_u32 n) { return dim3((n + 255u) / 256u); }

}  // namespace

extern "C" void agx_launch_evidence_gather(const agx_evidence_args *A, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_ev_gather, ev_grid(A->n + 1u), dim3(256), 0, st, *A);
    agx_launch_exclusive_scan(A->flag, A->foff, A->n, A->scan_tmp, st);
}

extern "C" void agx_launch_evidence_runs(const agx_evidence_args *A, hipStream_t st) {
    if (A->n && A->iv_cap) hipLaunchKernelGGL(agx_k_ev_runs, ev_grid(A->n), dim3(256), 0, st, *A);
}
