// agx_span.hip — gfx950 kernels of the pair span (agx_unit_pair_span, agx_unit_walk_span).
//
// A kept hit's two mates bound a fragment [f_lo, f_hi] (agx_span_fragment, agx_core.h).  span[x] counts the fragments across position x, cross[x] those across x and
// x + 1, pairs(x, y) those across x and y.  The per-position numbers are a scatter and a scan: every hit adds 1 where its fragment begins and 1 where it ends
// (agx_k_span_mark, clamped to the window the call works on), the running sum of start[x] - end[x - 1] is span (agx_k_span_diff, the multi-launch scan) and
// agx_k_span_finish leaves span and cross in place of start and end.  Under a stretch table a step between neighbouring positions is cross[x]; a step that jumps is counted
// over the hits against a sorted table of the jumps (agx_k_sp_jumps, agx_span_jump_walk).  The thin intervals are §14's: agx_k_sp_flags leaves what agx_k_ev_runs reads.
// All arithmetic is integer and every atomic returns nothing, so a result is the same run to run.  The kernels read the unit's arrays and write only the export's
// scratch; every index is held against the capacity of what it names before anything is read or stored there, and every loop runs to a count the kernel read.
#include <hip/hip_runtime.h>
#include "agx_kargs.h"

namespace {

constexpr unsigned long long SP_NONE64 = ~0ull;

__device__ __forceinline__ agx_u32 sp_sum32(agx_u32 v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long sp_sum64(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned long long sp_min64(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}

// the fragment of hit record i, the record read as five 8-byte words (the fifth, x_lo / x_hi, is not needed)
__device__ __forceinline__ int sp_fragment(const agx_dhit *dhit, agx_u32 i, const agx_run *runs, agx_u32 n_runs, agx_u32 n_pos, agx_u32 *f_lo, agx_u32 *f_hi) {
    const uint2 *g = reinterpret_cast<const uint2 *>(dhit + i);
    const uint2 w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3];
    return agx_span_fragment_v(w0.x, w0.y, w1.x, w1.y, w2.y & 0xFFFFu, w3.x & 0xFFFFu, w3.x >> 16, w3.y, runs, n_runs, n_pos, f_lo, f_hi);
}

// The mark pass: the lanes stride over all hit records.  A wavefront leaves its three counts as one partial; the host sums them.
__global__ void __launch_bounds__(256) agx_k_span_mark(agx_span_args A) {
    const agx_u32 stride = gridDim.x * 256u, wave = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    agx_u32 n_frag = 0, n_kept = 0, n_out = 0;
    for (agx_u32 base = blockIdx.x * 256u; base < A.n_hits; base += stride) {      // (wave-uniform: the wavefront's lanes leave the loop together)
        const agx_u32 i = base + threadIdx.x;
        if (i < A.n_hits) {
            agx_u32 f_lo, f_hi;
            const int kind = sp_fragment(A.dhit, i, A.runs, A.n_runs, A.n_pos, &f_lo, &f_hi);
            n_kept += kind != AGX_SPAN_SKIPPED ? 1u : 0u;
            n_out += kind == AGX_SPAN_OUTSIDE ? 1u : 0u;
            if (kind == AGX_SPAN_FRAGMENT) {
                agx_u32 s, e; bool has_end;
                n_frag += agx_span_clamp(f_lo, f_hi, A.win_lo, A.win_hi, &s, &e, &has_end) ? 1u : 0u;
                if (agx_span_clamp(f_lo, f_hi, A.lo, A.lo + A.n, &s, &e, &has_end)) {
                    if (s < A.n) atomicAdd(A.start + s, 1u);
                    if (has_end && e < A.n) atomicAdd(A.end + e, 1u);
                }
            }
        }
        if (stride > 0xFFFFFFFFu - base) break;      // (the next base would wrap)
    }
    n_frag = sp_sum32(n_frag); n_kept = sp_sum32(n_kept); n_out = sp_sum32(n_out);
    if (lane == 0 && wave < A.n_part) { A.part[3u * wave] = n_frag; A.part[3u * wave + 1u] = n_kept; A.part[3u * wave + 2u] = n_out; }
}

// start[x] -= end[x - 1] (wrapping; the running sum is exact: every true value is below the number of hits).  In place: a thread reads and writes its own entry of start.
__global__ void __launch_bounds__(256) agx_k_span_diff(agx_span_args A) {
    const agx_u32 x = blockIdx.x * 256u + threadIdx.x;
    if (x > 0 && x < A.n) A.start[x] -= A.end[x - 1u];
}

// span[x] = the running sum up to and including x = sc[x + 1]; cross[x] = span[x] less the fragments that end on x.  In place of start and end.
__global__ void __launch_bounds__(256) agx_k_span_finish(agx_span_args A) {
    const agx_u32 x = blockIdx.x * 256u + threadIdx.x;
    if (x >= A.n) return;
    const agx_u32 span = A.sc[x + 1u];
    A.start[x] = span; A.end[x] = span - A.end[x];
}

// ---- under the walk's records --------------------------------------------------------------------------------------------------

// The gather: per base of the chunk its position, its span and — a step between neighbouring positions — its step; a jump is flagged, a step that is not forward counted.
// A thread per flat base of the chunk and one more for the flags' closing zero.
__global__ void __launch_bounds__(256) agx_k_sp_gather(agx_walk_span_args A) {
    const agx_evidence_args &E = A.E;
    const agx_u32 j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = j < E.n;
    agx_evidence_base b{AGX_NONE, AGX_NONE, 0u, AGX_NONE, AGX_NONE, AGX_NONE, AGX_NONE, AGX_NONE, false, false};
    if (in) b = agx_evidence_lane(E.T, E.lo + j);
    const bool valid = in && b.st != AGX_NONE;
    const agx_u32 x = valid ? agx_span_pos(b.id, A.n_pos, E.T.n_ids, A.side_xpos) : AGX_NONE;
    // the step's target: the neighbour lane's position where the step stays inside the stretch and the neighbour is a lane of this wavefront and a base of this chunk
    const agx_u32 nb = __shfl_down(x, 1, 64);
    agx_u32 step = AGX_NONE, jump = 0u;
    if (valid && b.has_step) {
        const agx_u32 y = b.inner && lane < 63u && j + 1u < E.n ? nb : agx_span_pos(b.next_id, A.n_pos, E.T.n_ids, A.side_xpos);
        const int kind = agx_span_step_kind(x, y);
        if (kind == AGX_SPAN_STEP_NEXT) step = A.cross[x];      // (x < y < n_pos or NONE: agx_span_pos; NONE is never NEXT)
        else if (kind == AGX_SPAN_STEP_JUMP) jump = 1u;
        else atomicAdd(E.noedge, 1u);
    }
    if (valid) { A.c_pos[j] = x; E.c_depth[j] = x < A.n_pos ? A.span[x] : AGX_NONE; E.c_step[j] = step; }
    if (j <= E.n) A.jflag[j] = jump;
}

// The jump list: a flagged base writes (x, y, flat base) at the place the flags' scan gives it.
__global__ void __launch_bounds__(256) agx_k_sp_emit(agx_walk_span_args A) {
    const agx_evidence_args &E = A.E;
    const agx_u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j >= E.n || !A.jflag[j]) return;
    const agx_u32 at = A.joff[j];
    if (at >= A.jt_cap) { atomicOr(E.err, 2u); return; }
    const agx_evidence_base b = agx_evidence_lane(E.T, E.lo + j);
    if (b.st == AGX_NONE || !b.has_step) { atomicOr(E.err, 2u); return; }
    A.jt_x[at] = A.c_pos[j]; A.jt_y[at] = agx_span_pos(b.next_id, A.n_pos, E.T.n_ids, A.side_xpos); A.jt_base[at] = E.lo + j;
}

// The count: the lanes stride over all hit records; a fragment adds 1 to every entry it spans.
__global__ void __launch_bounds__(256) agx_k_sp_jumps(agx_walk_span_args A) {
    const agx_u32 stride = gridDim.x * 256u;
    for (agx_u32 base = blockIdx.x * 256u; base < A.n_hits; base += stride) {
        const agx_u32 i = base + threadIdx.x;
        if (i < A.n_hits) {
            agx_u32 f_lo, f_hi;
            if (sp_fragment(A.dhit, i, A.runs, A.n_runs, A.n_pos, &f_lo, &f_hi) == AGX_SPAN_FRAGMENT)
                agx_span_jump_walk(A.e_x, A.e_y, A.n_ent, f_lo, f_hi, [&](agx_u32 e) { atomicAdd(A.e_cnt + e, 1u); });
        }
        if (stride > 0xFFFFFFFFu - base) break;
    }
}

// every listed jump takes its entry's count as its base's step
__global__ void __launch_bounds__(256) agx_k_sp_scatter(agx_walk_span_args A) {
    const agx_u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k >= A.n_list) return;
    const agx_u32 fb = A.l_base[k], e = A.l_ent[k];
    if (e >= A.n_ent || fb < A.E.lo || fb - A.E.lo >= A.E.n) { atomicOr(A.E.err, 4u); return; }
    A.E.c_step[fb - A.E.lo] = A.e_cnt[e];
}

// The record summaries and the interval-start flags of the chunk, from the per-base numbers (agx_k_ev_gather's second half with span for depth).  A thread per flat base of
// the chunk and one more for the flags' closing zero.
__global__ void __launch_bounds__(256) agx_k_sp_flags(agx_walk_span_args A) {
    const agx_evidence_args &E = A.E;
    const agx_u32 j = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = j < E.n;
    agx_evidence_base b{AGX_NONE, AGX_NONE, 0u, AGX_NONE, AGX_NONE, AGX_NONE, AGX_NONE, AGX_NONE, false, false};
    if (in) b = agx_evidence_lane(E.T, E.lo + j);
    const bool valid = in && b.st != AGX_NONE;
    const agx_u32 span = valid ? E.c_depth[j] : AGX_NONE, step = valid ? E.c_step[j] : AGX_NONE;
    const bool weak = valid && agx_evidence_weak(span, step, E.min_depth, E.min_support);
    // interval starts: thin, and the flat base in front is not a thin base of the same record at offset - 1.  The chunk's first base has nothing in front: an interval
    // cut by the chunk's border is merged on the host
    bool p_weak = __shfl_up((int)weak, 1, 64) != 0; agx_u32 p_rec = __shfl_up(b.rec, 1, 64), p_off = __shfl_up(b.off, 1, 64);
    if (lane == 0) {
        p_weak = false;
        if (valid && j > 0) {
            const agx_evidence_base p = agx_evidence_lane(E.T, E.lo + j - 1u);
            if (p.st != AGX_NONE) { p_rec = p.rec; p_off = p.off; p_weak = agx_evidence_weak(E.c_depth[j - 1u], E.c_step[j - 1u], E.min_depth, E.min_support); }
        }
    }
    if (j <= E.n) E.flag[j] = weak && !(p_weak && p_rec == b.rec && p_off + 1u == b.off) ? 1u : 0u;

    // record summaries: where the wavefront's bases belong to one record, one reduction and one atomic per quantity from lane 0, else per-lane atomics
    const bool rec_ok = valid && b.rec < E.n_recs;
    const unsigned long long steps = rec_ok && step != AGX_NONE ? 1ull : 0ull, ssum = rec_ok && span != AGX_NONE ? (unsigned long long)span : 0ull;
    const unsigned long long dkey = rec_ok && span != AGX_NONE ? ((unsigned long long)span << 32) | b.off : SP_NONE64;
    const unsigned long long skey = rec_ok && step != AGX_NONE ? ((unsigned long long)step << 32) | b.off : SP_NONE64;
    const agx_u32 r0 = __shfl(b.rec, 0, 64);
    const bool first_ok = __shfl((int)rec_ok, 0, 64) != 0;
    if (first_ok && __all(!rec_ok || b.rec == r0)) {
        const unsigned long long ts = sp_sum64(steps), td = sp_sum64(ssum), md = sp_min64(dkey), ms = sp_min64(skey);
        if (lane == 0) {
            if (ts) atomicAdd(E.r_steps + r0, ts);
            if (td) atomicAdd(E.r_dsum + r0, td);
            if (md != SP_NONE64) atomicMin(E.r_dmin + r0, md);
            if (ms != SP_NONE64) atomicMin(E.r_smin + r0, ms);
        }
    } else if (rec_ok) {
        if (steps) atomicAdd(E.r_steps + b.rec, steps);
        if (ssum) atomicAdd(E.r_dsum + b.rec, ssum);
        if (dkey != SP_NONE64) atomicMin(E.r_dmin + b.rec, dkey);
        if (skey != SP_NONE64) atomicMin(E.r_smin + b.rec, skey);
    }
}

inline dim3 sp_grid(agx_u32 n) { return dim3((n + 255u) / 256u); }
inline agx_u32 sp_hit_blocks(agx_u32 n_hits) { const agx_u32 b = n_hits / 256u + (n_hits % 256u ? 1u : 0u); return b < 1u ? 1u : b > AGX_SPAN_BLOCKS ? AGX_SPAN_BLOCKS : b; }      // (n_hits + 255 would wrap within 255 of 2^32)

}  // namespace

extern "C" agx_u32 agx_span_partials(agx_u32 n_hits) { return sp_hit_blocks(n_hits) * 4u; }

extern "C" void agx_launch_pair_span(const agx_span_args *A, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_span_mark, dim3(sp_hit_blocks(A->n_hits)), dim3(256), 0, st, *A);
    if (A->n > 1u) hipLaunchKernelGGL(agx_k_span_diff, sp_grid(A->n), dim3(256), 0, st, *A);
    agx_launch_exclusive_scan(A->start, A->sc, A->n, A->scan_tmp, st);
    if (A->n) hipLaunchKernelGGL(agx_k_span_finish, sp_grid(A->n), dim3(256), 0, st, *A);
}

extern "C" void agx_launch_walk_span_gather(const agx_walk_span_args *A, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_sp_gather, sp_grid(A->E.n + 1u), dim3(256), 0, st, *A);
    agx_launch_exclusive_scan(A->jflag, A->joff, A->E.n, A->E.scan_tmp, st);
}

extern "C" void agx_launch_walk_span_emit(const agx_walk_span_args *A, hipStream_t st) {
    if (A->E.n && A->jt_cap) hipLaunchKernelGGL(agx_k_sp_emit, sp_grid(A->E.n), dim3(256), 0, st, *A);
}

extern "C" void agx_launch_walk_span_jumps(const agx_walk_span_args *A, hipStream_t st) {
    if (!A->n_ent || !A->n_list) return;
    if (A->n_hits) hipLaunchKernelGGL(agx_k_sp_jumps, dim3(sp_hit_blocks(A->n_hits)), dim3(256), 0, st, *A);
    hipLaunchKernelGGL(agx_k_sp_scatter, sp_grid(A->n_list), dim3(256), 0, st, *A);
}

extern "C" void agx_launch_walk_span_flags(const agx_walk_span_args *A, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_sp_flags, sp_grid(A->E.n + 1u), dim3(256), 0, st, *A);
    agx_launch_exclusive_scan(A->E.flag, A->E.foff, A->E.n, A->E.scan_tmp, st);
}
