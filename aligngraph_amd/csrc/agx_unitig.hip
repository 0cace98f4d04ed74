// agx_unitig.hip — gfx950 kernels of the unitig export (agx_unit_unitigs).
//
// They read the node table a build leaves in HBM (node_start / node_cnt, n_flags, n_next with the overflow list, n_base, the counts, ref) and write
// only their own scratch.  A node is alive when the build did not prune it (AGX_NF_DEAD clear); an alive edge joins two alive nodes; an edge u -> v is
// INTERNAL when u has one alive successor, v one alive predecessor and u != v; a unitig is a maximal path of internal edges.  Every edge the build
// makes goes from a position to a later one, so the alive graph is a DAG and every unitig has one head; the degree kernels check that where they
// look at the edges anyway and set a bit of the error word instead of trusting it.
//
// Shape: one pass over positions for degrees and internal edges; the nodes in slot order, a wavefront per 64 slots, cut into PIECES (runs of
// u -> u+1 internal edges inside the window: the common case, since a position's single variant sits one slot behind its predecessor's); the
// pieces ranked by pointer jumping in ceil(log2 pieces) + 1 rounds (no spins, no grid-wide barrier); heads compacted in (position, variant) order
// by a scan over positions; segment lengths and link counts scanned for the offsets; then every node writes its base and every tail its links.
// Every loop is bounded by a count the kernel read, and every store is checked against the capacity of what it writes.  The scans are the multi-launch
// form (agx_launch_exclusive_scan): nothing here spins, whatever builds run beside an export on the same device.
//
// The region export (agx_unit_unitigs_region; the agx_k_utr_* kernels in the second half of the file) applies the same definition to the nodes of a window of positions
// that are alive at a coverage of the caller's choice, over dense local ids instead of slots: none of its grids is sized by the unit.  What the two forms do to one node,
// one window or one overflow entry is written once, over a VIEW (ut_slots, ut_locals) that says how the form names its nodes; the kernels differ in their grids.
#include <hip/hip_runtime.h>
#include "agx_kargs.h"

namespace {

__device__ __forceinline__ bool ut_alive(const agx_unitig_args &A, agx_u32 slot) { return !(A.n_flags[slot] & AGX_NF_DEAD); }
__device__ __forceinline__ bool utr_kept(const agx_unitig_region_args &R, agx_u32 slot) {      // AG:1904-1918 with the caller's threshold
    return R.nk_cid[slot] != AGX_NONE || (long long)R.U.n_counts[(size_t)slot * 6] >= (long long)R.min_cov;
}

// A view: how an export names its nodes.  args(): the per-id arrays; slot_cap(): the unit's node slots; in_export(slot): the id of a slot's node, NONE if the slot is
// outside the pool or its node is not in the export; slot_of(id): the slot of a node of the export; valid(id): whether the id names one.
// The whole export: a node's id is its slot, and it is in the export unless the build pruned it
struct ut_slots {
    const agx_unitig_args &A;
    __device__ __forceinline__ const agx_unitig_args &args() const { return A; }
    __device__ __forceinline__ agx_u32 slot_cap() const { return A.pool_cap; }
    __device__ __forceinline__ agx_u32 in_export(agx_u32 slot) const { return slot < A.pool_cap && ut_alive(A, slot) ? slot : AGX_NONE; }
    __device__ __forceinline__ agx_u32 slot_of(agx_u32 id) const { return id; }
    __device__ __forceinline__ bool valid(agx_u32 id) const { return id < A.pool_cap && A.pos_of[id] != AGX_NONE && ut_alive(A, id); }
};
// The region export: dense local ids (l_slot: id -> slot; rmap: slot -> id).  rmap holds whatever the last export of any kind left in it: an entry counts only if the
// local id it names points back at the slot
struct ut_locals {
    const agx_unitig_region_args &R;
    __device__ __forceinline__ const agx_unitig_args &args() const { return R.U; }
    __device__ __forceinline__ agx_u32 slot_cap() const { return R.pool_cap; }
    __device__ __forceinline__ agx_u32 in_export(agx_u32 slot) const {
        if (slot >= R.pool_cap) return AGX_NONE;
        const agx_u32 r = R.rmap[slot];
        return r < R.U.pool_cap && R.l_slot[r] == slot ? r : AGX_NONE;
    }
    __device__ __forceinline__ agx_u32 slot_of(agx_u32 id) const { return R.l_slot[id]; }
    __device__ __forceinline__ bool valid(agx_u32 id) const { return id < R.U.pool_cap; }
};

// ---- the steps both forms take, over a view -------------------------------------------------------------------------------------------------------------------

// entry i of the overflow list: an edge may be listed more than once (two lanes that inserted it at the same time); the first to enter the hash set counts it
template <class V> __device__ __forceinline__ void ut_ovf_insert(const V &v, agx_u32 i) {
    const agx_unitig_args &A = v.args();
    if (i >= A.n_ovf) return;
    A.ovf_first[i] = 0;
    const agx_u32 s = A.ovf[i].src, d = A.ovf[i].dst;
    if (s == AGX_NONE || d == AGX_NONE) return;
    if (s >= v.slot_cap() || d >= v.slot_cap()) { atomicOr(A.err, 2u); return; }
    const agx_u32 ls = v.in_export(s), ld = v.in_export(d);
    if (ls == AGX_NONE || ld == AGX_NONE) return;
    const agx_u32 sp = A.pos_of[ls], dp = A.pos_of[ld];
    if (sp == AGX_NONE || dp == AGX_NONE || dp <= sp) { atomicOr(A.err, 1u); return; }
    const unsigned long long key = ((unsigned long long)ls << 32) | ld;
    agx_u32 h = (agx_u32)((key * 0x9E3779B97F4A7C15ull) >> 32) & A.hash_mask;
    for (agx_u32 probe = 0; probe <= A.hash_mask; probe++) {          // (the set holds twice the list: a free cell is always found)
        const unsigned long long old = atomicCAS(A.ovf_hash + h, ~0ull, key);
        if (old == key) return;
        if (old == ~0ull) {
            A.ovf_first[i] = 1;
            atomicAdd(A.indeg + ld, 1u); atomicAdd(A.oout + ls, 1u); A.osucc[ls] = ld;      // (osucc is only read where oout == 1)
            return;
        }
        h = (h + 1u) & A.hash_mask;
    }
}

// the internal edge of node id (in: it is a node of the export): nxt[id] = the one successor if that has one predecessor; outs[id] becomes the whole out-degree
__device__ __forceinline__ void ut_internal_of(const agx_unitig_args &A, agx_u32 id, bool in) {
    agx_u32 nx = AGX_NONE;
    if (in) {
        const agx_u32 a = A.outs[id], b = A.oout[id], d = a + b;
        const agx_u32 t = d != 1u ? AGX_NONE : a == 1u ? A.succ[id] : A.osucc[id];
        if (t != AGX_NONE && t < A.pool_cap && A.indeg[t] == 1u) { nx = t; A.haspred[t] = 1; }
        A.outs[id] = d;
    }
    A.nxt[id] = nx; A.succ[id] = AGX_NONE;          // (succ becomes the piece id of piece starts)
}

// 64 consecutive ids, a lane each: which lanes are nodes of the export, which continue into the next id (internal edge u -> u+1), which start a piece
struct ut_window { agx_u32 u, lane, nx; bool valid, link; unsigned long long lm, sm; };
template <class V> __device__ __forceinline__ ut_window ut_window_of(const V &v) {
    const agx_unitig_args &A = v.args();
    ut_window w;
    w.u = blockIdx.x * 256u + threadIdx.x; w.lane = threadIdx.x & 63u;
    w.valid = v.valid(w.u);
    w.nx = w.valid ? A.nxt[w.u] : AGX_NONE;
    w.link = w.valid && w.lane < 63u && w.nx == w.u + 1u;
    w.lm = __ballot(w.link);
    const bool prev = w.lane > 0 && ((w.lm >> (w.lane - 1u)) & 1ull);
    w.sm = __ballot(w.valid && !prev);
    return w;
}

// the window's pieces: each one's length, the id its last node's internal edge enters, and its piece id at its first node
// (the ids come from a scan of the windows' counts: one atomic counter per wavefront cost 5.6 ms on a 30 Mb unit, every wavefront waiting for the same address)
__device__ __forceinline__ void ut_cut(const agx_unitig_args &A, const ut_window &w) {
    const bool start = (w.sm >> w.lane) & 1ull;
    const agx_u32 end = w.lane + (agx_u32)__builtin_ctzll(~w.lm >> w.lane);      // (bit 63 of ~lm is always set)
    const agx_u32 nx_end = __shfl(w.nx, (int)end, 64);
    if (!start) return;
    const agx_u32 pid = A.woff[w.u / 64u] + (agx_u32)__popcll(w.sm & ((1ull << w.lane) - 1ull));
    if (pid >= A.piece_cap) { atomicOr(A.err, 4u); return; }
    A.p_len[pid] = end - w.lane + 1u; A.p_next[pid] = nx_end; A.succ[w.u] = pid;
}

// every node: its segment and rank; every tail: its segment's length, last position and link count; coverage summed per piece, one atomic per piece
template <class V> __device__ __forceinline__ void ut_rank_of(const V &v, agx_u32 np, agx_u32 fin) {
    const agx_unitig_args &A = v.args();
    const ut_window w = ut_window_of(v);
    const unsigned long long below = w.sm & ((2ull << w.lane) - 1ull);
    const agx_u32 ps = below ? 63u - (agx_u32)__builtin_clzll(below) : 0u;
    const bool start = (w.sm >> w.lane) & 1ull;
    const agx_u32 pid_here = start ? A.succ[w.u] : AGX_NONE;
    const agx_u32 pid = __shfl(pid_here, (int)ps, 64);
    const agx_u32 slot = w.valid ? v.slot_of(w.u) : AGX_NONE;
    unsigned long long cov = slot < v.slot_cap() ? (unsigned long long)(agx_u32)A.n_counts[(size_t)slot * 6] : 0ull, incl = cov;
    for (agx_u32 d = 1; d < 64u; d <<= 1) { const unsigned long long o = __shfl_up(incl, d, 64); if (w.lane >= d) incl += o; }
    const unsigned long long excl_ps = __shfl(incl - cov, (int)ps, 64);
    if (!w.valid) return;
    if (pid >= np) { atomicOr(A.err, 4u); return; }
    const agx_u32 h = A.anc[fin][pid];
    if (h >= np || A.anc[fin][h] != h) { atomicOr(A.err, 4u); return; }       // (not converged: impossible on a DAG)
    const agx_u32 seg = A.p_seg[h];
    if (seg >= A.piece_cap) { atomicOr(A.err, 4u); return; }
    const agx_u32 rank = A.off[fin][pid] + (w.lane - ps);
    A.indeg[w.u] = seg; A.osucc[w.u] = rank;
    if (!w.link) atomicAdd(A.s_cov + seg, incl - excl_ps);            // the piece's last node
    if (w.nx == AGX_NONE) { A.s_len[seg] = rank + 1u; A.s_last[seg] = A.pos_of[w.u]; A.s_links[seg] = A.outs[w.u]; }
}

// node id at position X (ns: the segments): its base at s_off[seg] + rank; a tail's inline links (the overflow list's follow in ut_ovf_link)
template <class V> __device__ __forceinline__ void ut_emit_node(const V &v, agx_u32 id, agx_u32 X, agx_u32 ns) {
    const agx_unitig_args &A = v.args();
    const agx_u32 seg = A.indeg[id], rank = A.osucc[id], u = v.slot_of(id);
    if (seg >= ns || u >= v.slot_cap()) { atomicOr(A.err, 4u); return; }
    const agx_u32 at = A.s_off[seg] + rank;
    const char c = (char)A.n_base[u];
    if (at < A.s_off[seg + 1] && at < A.seq_cap) A.seq[at] = c != 'X' ? c : A.ref[X];       // consensus, else the reference base (AG:1997-2001)
    else atomicOr(A.err, 4u);
    if (A.nxt[id] != AGX_NONE) return;
    const agx_u32 lo = A.l_off[seg], hi = A.l_off[seg + 1];
    const uint4 nx = *reinterpret_cast<const uint4 *>(A.n_next + (size_t)u * AGX_MAXE);
    const agx_u32 t[AGX_MAXE] = {nx.x, nx.y, nx.z, nx.w};
    agx_u32 k = 0;
    for (agx_u32 e = 0; e < AGX_MAXE; e++) {
        const agx_u32 lt = v.in_export(t[e]);          // (NONE is no slot)
        if (lt == AGX_NONE) continue;
        if (lo + k < hi && lo + k < A.link_cap) A.l_to[lo + k] = A.indeg[lt]; else atomicOr(A.err, 4u);
        k++;
    }
    A.l_cur[seg] = k;
}

// the link of an overflow edge s -> d (ids of two nodes of the export) that is the first of its kind on the list
__device__ __forceinline__ void ut_ovf_link(const agx_unitig_args &A, agx_u32 s, agx_u32 d) {
    if (A.nxt[s] == d) return;                                          // the internal edge of a node whose only successor is on the list
    const agx_u32 seg = A.indeg[s], ns = A.hoff[A.n_pos];
    if (seg >= ns) { atomicOr(A.err, 4u); return; }
    const agx_u32 at = A.l_off[seg] + atomicAdd(A.l_cur + seg, 1u);
    if (at < A.l_off[seg + 1] && at < A.link_cap) A.l_to[at] = A.indeg[d]; else atomicOr(A.err, 4u);
}

// ---- whole export: a thread per position over its variants, or a wavefront per 64 slots -------------------------------------------------------------------------

// pos_of[slot] for every used slot (pos_of was set to NONE before)
__global__ void __launch_bounds__(256) agx_k_ut_pos(agx_unitig_args A) {
    const agx_u32 X = blockIdx.x * 256u + threadIdx.x;
    if (X >= A.n_pos) return;
    const agx_u32 s = A.node_start[X], n = A.node_cnt[X];
    for (agx_u32 v = 0; v < n; v++) {
        if (s + v >= A.pool_cap) { atomicOr(A.err, 2u); return; }
        A.pos_of[s + v] = X;
    }
}

// alive successors among the inline slots (distinct by construction: the build inserts into them as a set) and the in-degree they give
__global__ void __launch_bounds__(256) agx_k_ut_degrees(agx_unitig_args A) {
    const agx_u32 X = blockIdx.x * 256u + threadIdx.x;
    if (X >= A.n_pos) return;
    const agx_u32 s = A.node_start[X], n = A.node_cnt[X];
    for (agx_u32 v = 0; v < n && s + v < A.pool_cap; v++) {
        const agx_u32 u = s + v;
        if (!ut_alive(A, u)) continue;
        const uint4 nx = *reinterpret_cast<const uint4 *>(A.n_next + (size_t)u * AGX_MAXE);
        const agx_u32 t[AGX_MAXE] = {nx.x, nx.y, nx.z, nx.w};
        agx_u32 cnt = 0, last = AGX_NONE;
        for (agx_u32 e = 0; e < AGX_MAXE; e++) {
            if (t[e] == AGX_NONE) continue;
            if (t[e] >= A.pool_cap) { atomicOr(A.err, 2u); continue; }
            if (!ut_alive(A, t[e])) continue;
            const agx_u32 tp = A.pos_of[t[e]];
            if (tp == AGX_NONE || tp <= X) { atomicOr(A.err, 1u); continue; }
            cnt++; last = t[e];
            atomicAdd(A.indeg + t[e], 1u);
        }
        A.outs[u] = cnt; A.succ[u] = last;
    }
}
__global__ void __launch_bounds__(256) agx_k_ut_ovf(agx_unitig_args A) { ut_ovf_insert(ut_slots{A}, blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) agx_k_ut_internal(agx_unitig_args A) {
    const agx_u32 X = blockIdx.x * 256u + threadIdx.x;
    if (X >= A.n_pos) return;
    const agx_u32 s = A.node_start[X], n = A.node_cnt[X];
    for (agx_u32 v = 0; v < n && s + v < A.pool_cap; v++) ut_internal_of(A, s + v, ut_alive(A, s + v));
}

__global__ void __launch_bounds__(256) agx_k_ut_piece_count(agx_unitig_args A) {
    const ut_window w = ut_window_of(ut_slots{A});
    if (w.lane == 0 && w.u < A.pool_cap) A.wcnt[w.u / 64u] = (agx_u32)__popcll(w.sm);
}
__global__ void __launch_bounds__(256) agx_k_ut_pieces(agx_unitig_args A) { ut_cut(A, ut_window_of(ut_slots{A})); }

// pointer jumping over the pieces: anc = predecessor piece (self for a head), off = nodes of the predecessor
__global__ void __launch_bounds__(256) agx_k_ut_jump_init(agx_unitig_args A, agx_u32 np) {
    const agx_u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= np) return;
    A.anc[0][p] = p; A.off[0][p] = 0;
}
__global__ void __launch_bounds__(256) agx_k_ut_jump_link(agx_unitig_args A, agx_u32 np) {
    const agx_u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= np) return;
    const agx_u32 t = A.p_next[p];
    if (t == AGX_NONE) return;
    const agx_u32 q = t < A.pool_cap ? A.succ[t] : AGX_NONE;       // (the target of an internal edge that leaves a piece always starts one)
    if (q >= np) { atomicOr(A.err, 4u); return; }
    A.anc[0][q] = p; A.off[0][q] = A.p_len[p];
}
__global__ void __launch_bounds__(256) agx_k_ut_jump(agx_unitig_args A, agx_u32 np, agx_u32 r) {
    const agx_u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= np) return;
    const agx_u32 *ai = A.anc[r & 1u], *oi = A.off[r & 1u];
    agx_u32 *ao = A.anc[(r & 1u) ^ 1u], *oo = A.off[(r & 1u) ^ 1u];
    const agx_u32 a = ai[p];
    if (a == p || a >= np) { ao[p] = a; oo[p] = oi[p]; return; }
    ao[p] = ai[a]; oo[p] = oi[p] + oi[a];
}

// heads: alive nodes without an internal predecessor, counted per position and numbered in (position, variant) order
__global__ void __launch_bounds__(256) agx_k_ut_head_count(agx_unitig_args A) {
    const agx_u32 X = blockIdx.x * 256u + threadIdx.x;
    if (X >= A.n_pos) return;
    const agx_u32 s = A.node_start[X], n = A.node_cnt[X];
    agx_u32 c = 0;
    for (agx_u32 v = 0; v < n && s + v < A.pool_cap; v++) c += (ut_alive(A, s + v) && !A.haspred[s + v]) ? 1u : 0u;
    A.hcnt[X] = c;
}
__global__ void __launch_bounds__(256) agx_k_ut_head_assign(agx_unitig_args A, agx_u32 np) {
    const agx_u32 X = blockIdx.x * 256u + threadIdx.x;
    if (X >= A.n_pos) return;
    const agx_u32 s = A.node_start[X], n = A.node_cnt[X];
    agx_u32 seg = A.hoff[X];
    for (agx_u32 v = 0; v < n && s + v < A.pool_cap; v++) {
        const agx_u32 u = s + v;
        if (!ut_alive(A, u) || A.haspred[u]) continue;
        const agx_u32 p = A.succ[u];
        if (p >= np || seg >= A.piece_cap) { atomicOr(A.err, 4u); return; }
        A.p_seg[p] = seg; A.s_hpos[seg] = X; A.s_hvar[seg] = v;
        seg++;
    }
}
__global__ void __launch_bounds__(256) agx_k_ut_rank(agx_unitig_args A, agx_u32 np, agx_u32 fin) { ut_rank_of(ut_slots{A}, np, fin); }

__global__ void agx_k_ut_totals(agx_unitig_args A, agx_u32 *tot) {
    if (threadIdx.x || blockIdx.x) return;
    const agx_u32 ns = A.hoff[A.n_pos];
    tot[0] = ns; tot[1] = ns <= A.piece_cap ? A.s_off[ns] : 0u; tot[2] = ns <= A.piece_cap ? A.l_off[ns] : 0u; tot[3] = *A.err;
}

__global__ void __launch_bounds__(256) agx_k_ut_emit(agx_unitig_args A) {
    const agx_u32 X = blockIdx.x * 256u + threadIdx.x;
    if (X >= A.n_pos) return;
    const agx_u32 s = A.node_start[X], n = A.node_cnt[X];
    const agx_u32 ns = A.hoff[A.n_pos];
    for (agx_u32 v = 0; v < n && s + v < A.pool_cap; v++)
        if (ut_alive(A, s + v)) ut_emit_node(ut_slots{A}, s + v, X, ns);
}
__global__ void __launch_bounds__(256) agx_k_ut_links_ovf(agx_unitig_args A) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_ovf || !A.ovf_first[i]) return;
    ut_ovf_link(A, A.ovf[i].src, A.ovf[i].dst);                        // (both alive and in the pool: agx_k_ut_ovf)
}
// each segment's links by target segment (link_from is filled on the host from the offsets) (a few per tail; the overflow list's nodes have more), insertion sort in the segment's own range
__global__ void __launch_bounds__(256) agx_k_ut_links_sort(agx_unitig_args A) {
    const agx_u32 g = blockIdx.x * 256u + threadIdx.x;
    const agx_u32 ns = A.hoff[A.n_pos];
    if (g >= ns) return;
    const agx_u32 lo = A.l_off[g], hi = A.l_off[g + 1] < A.link_cap ? A.l_off[g + 1] : A.link_cap;
    for (agx_u32 i = lo; i < hi; i++) {
        const agx_u32 x = A.l_to[i];
        agx_u32 j = i;
        while (j > lo && A.l_to[j - 1] > x) { A.l_to[j] = A.l_to[j - 1]; j--; }
        A.l_to[j] = x;
    }
}

// ---- region export (agx_unit_unitigs_region, agx_kargs.h: agx_unitig_region_args) -------------------------------------------------------------------------
// The same graph definition on a sub-graph: the nodes of the window's positions that are alive at the caller's coverage, and the edges between two of them.  No grid below
// is sized by the unit: one thread per position of the window (count, compact), per kept node (everything else) or per overflow entry (the list has no position index).
// Kept nodes are numbered densely in (position, variant) order, so a wavefront takes 64 consecutive local ids, "the internal edge goes to the next id" is the common case
// as it is for slots in the whole export, and heads are numbered by a scan over the 64-id groups.  R.U is the local view the jumping, totals and link-sort kernels run on unchanged.

__global__ void __launch_bounds__(256) agx_k_utr_count(agx_unitig_region_args R) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i > R.n_win) return;
    agx_u32 c = 0;
    if (i < R.n_win) {
        const agx_u32 X = R.pos_lo + i, s = R.U.node_start[X], n = R.node_cnt[X];
        for (agx_u32 v = 0; v < n; v++) {
            if (s + v >= R.pool_cap) { atomicOr(R.U.err, 2u); break; }
            c += utr_kept(R, s + v) ? 1u : 0u;
        }
    }
    R.cntw[i] = c;                  // (entry n_win: the scan's closing zero)
}
// local ids: slot and position of each, the reverse map at its slot, and the zeros the degree kernels add to
__global__ void __launch_bounds__(256) agx_k_utr_compact(agx_unitig_region_args R) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= R.n_win) return;
    const agx_u32 X = R.pos_lo + i, s = R.U.node_start[X], n = R.node_cnt[X];
    agx_u32 id = R.offw[i];
    for (agx_u32 v = 0; v < n && s + v < R.pool_cap; v++) {
        if (!utr_kept(R, s + v)) continue;
        if (id >= R.U.pool_cap) { atomicOr(R.U.err, 4u); return; }
        R.l_slot[id] = s + v; R.U.pos_of[id] = X; R.rmap[s + v] = id;
        R.U.indeg[id] = 0; R.U.oout[id] = 0; R.U.haspred[id] = 0;
        id++;
    }
}
__global__ void __launch_bounds__(256) agx_k_utr_degrees(agx_unitig_region_args R) {
    const agx_u32 id = blockIdx.x * 256u + threadIdx.x;
    if (id >= R.U.pool_cap) return;
    const agx_u32 u = R.l_slot[id], X = R.U.pos_of[id];
    agx_u32 cnt = 0, last = AGX_NONE;
    if (u < R.pool_cap) {
        const uint4 nx = *reinterpret_cast<const uint4 *>(R.U.n_next + (size_t)u * AGX_MAXE);
        const agx_u32 t[AGX_MAXE] = {nx.x, nx.y, nx.z, nx.w};
        for (agx_u32 e = 0; e < AGX_MAXE; e++) {
            if (t[e] == AGX_NONE) continue;
            if (t[e] >= R.pool_cap) { atomicOr(R.U.err, 2u); continue; }
            const agx_u32 lt = ut_locals{R}.in_export(t[e]);
            if (lt == AGX_NONE) continue;                                    // pruned at this threshold, or across the window's border
            if (R.U.pos_of[lt] <= X) { atomicOr(R.U.err, 1u); continue; }
            cnt++; last = lt;
            atomicAdd(R.U.indeg + lt, 1u);
        }
    } else atomicOr(R.U.err, 2u);
    R.U.outs[id] = cnt; R.U.succ[id] = last;
}
__global__ void __launch_bounds__(256) agx_k_utr_ovf(agx_unitig_region_args R) { ut_ovf_insert(ut_locals{R}, blockIdx.x * 256u + threadIdx.x); }
__global__ void __launch_bounds__(256) agx_k_utr_internal(agx_unitig_region_args R) {
    const agx_u32 id = blockIdx.x * 256u + threadIdx.x;
    if (id < R.U.pool_cap) ut_internal_of(R.U, id, true);
}

// pieces and heads per group (a head starts a piece: a lane behind a link has an internal predecessor)
__global__ void __launch_bounds__(256) agx_k_utr_group_count(agx_unitig_region_args R) {
    const ut_window w = ut_window_of(ut_locals{R});      // (64 consecutive local ids: all of them nodes of the export, up to the last group's tail)
    const unsigned long long hm = __ballot(w.valid && !R.U.haspred[w.valid ? w.u : 0u]);
    if (w.lane == 0 && w.valid) { R.U.wcnt[w.u / 64u] = (agx_u32)__popcll(w.sm); R.U.hcnt[w.u / 64u] = (agx_u32)__popcll(hm); }
}
__global__ void __launch_bounds__(256) agx_k_utr_pieces(agx_unitig_region_args R) { ut_cut(R.U, ut_window_of(ut_locals{R})); }
__global__ void __launch_bounds__(256) agx_k_utr_head_assign(agx_unitig_region_args R, agx_u32 np) {
    const agx_unitig_args &A = R.U;
    const agx_u32 u = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = u < A.pool_cap, head = valid && !A.haspred[valid ? u : 0u];
    const unsigned long long hm = __ballot(head);
    if (!head) return;
    const agx_u32 seg = A.hoff[u / 64u] + (agx_u32)__popcll(hm & ((1ull << lane) - 1ull)), p = A.succ[u];
    if (p >= np || seg >= A.piece_cap) { atomicOr(A.err, 4u); return; }
    const agx_u32 X = A.pos_of[u];
    A.p_seg[p] = seg; A.s_hpos[seg] = X; A.s_hvar[seg] = R.l_slot[u] - A.node_start[X];      // the variant index among ALL of the position's variants
}
__global__ void __launch_bounds__(256) agx_k_utr_rank(agx_unitig_region_args R, agx_u32 np, agx_u32 fin) { ut_rank_of(ut_locals{R}, np, fin); }
__global__ void __launch_bounds__(256) agx_k_utr_emit(agx_unitig_region_args R) {
    const agx_u32 id = blockIdx.x * 256u + threadIdx.x;
    if (id < R.U.pool_cap) ut_emit_node(ut_locals{R}, id, R.U.pos_of[id], R.U.hoff[R.U.n_pos]);
}
__global__ void __launch_bounds__(256) agx_k_utr_links_ovf(agx_unitig_region_args R) {
    const agx_unitig_args &A = R.U;
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_ovf || !A.ovf_first[i]) return;
    const agx_u32 s = A.ovf[i].src, d = A.ovf[i].dst;                 // (both in the pool and in the export: agx_k_utr_ovf; looked at again, since the ids have to be looked up anyway)
    if (s >= R.pool_cap || d >= R.pool_cap) { atomicOr(A.err, 4u); return; }
    const agx_u32 ls = ut_locals{R}.in_export(s), ld = ut_locals{R}.in_export(d);
    if (ls == AGX_NONE || ld == AGX_NONE) { atomicOr(A.err, 4u); return; }
    ut_ovf_link(A, ls, ld);
}

// the support of every link of a region export (agx_unit_unitigs_support), behind phase 3: a thread per kept node, the tails work.  Link i of the tail's segment enters
// segment l_to[i] at its head node (a node a link enters has no internal predecessor); the edge tail -> head sits in an inline slot of the tail, or — tails with
// AGX_NF_EOVF only — on the overflow list, whose duplicates are summed.  Every link is written by its one tail.
__global__ void __launch_bounds__(256) agx_k_utr_link_support(agx_unitig_region_args R, const agx_u8 *n_flags, const agx_u32 *e_cnt, const agx_u32 *ovf_cnt, agx_u32 *l_sup) {
    const agx_unitig_args &A = R.U;
    const agx_u32 id = blockIdx.x * 256u + threadIdx.x;
    if (id >= A.pool_cap || A.nxt[id] != AGX_NONE) return;
    const agx_u32 seg = A.indeg[id], ns = A.hoff[A.n_pos], u = R.l_slot[id];
    if (seg >= ns || u >= R.pool_cap) { atomicOr(A.err, 4u); return; }
    const agx_u32 lo = A.l_off[seg], hi = A.l_off[seg + 1] < A.link_cap ? A.l_off[seg + 1] : A.link_cap;
    const uint4 nx = *reinterpret_cast<const uint4 *>(A.n_next + (size_t)u * AGX_MAXE);
    const agx_u32 t[AGX_MAXE] = {nx.x, nx.y, nx.z, nx.w};
    const bool eovf = (n_flags[u] & AGX_NF_EOVF) != 0;
    for (agx_u32 i = lo; i < hi; i++) {
        const agx_u32 g = A.l_to[i];
        if (g >= ns) { atomicOr(A.err, 4u); continue; }
        const agx_u32 h = A.node_start[A.s_hpos[g]] + A.s_hvar[g];      // (s_hpos: a position of the window, written from pos_of)
        agx_u32 sum = 0;
        for (agx_u32 e = 0; e < AGX_MAXE; e++) sum += t[e] == h ? e_cnt[(size_t)u * AGX_MAXE + e] : 0u;
        if (eovf) for (agx_u32 j = 0; j < A.n_ovf; j++) sum += (A.ovf[j].src == u && A.ovf[j].dst == h) ? ovf_cnt[j] : 0u;
        l_sup[i] = sum;
    }
}

// ---- id map of a region export (agx_unit_unitigs_mapped, agx_kargs.h: agx_idmap_args) ------------------------------------------------------------------------
// One thread per window id; nothing is sized by the unit.  (segment, rank) per local id are the rank kernel's (U.indeg, U.osucc), which phase 3 only reads.

// side ids in front of position x: the first index of side_xpos (sorted) that holds x or more.  32 halvings at most
__device__ __forceinline__ agx_u32 idm_lower(const agx_u32 *xs, agx_u32 n, agx_u32 x) {
    agx_u32 lo = 0, hi = n;
    for (agx_u32 it = 0; it < 32u && lo < hi; it++) { const agx_u32 mid = lo + (hi - lo) / 2u; if (xs[mid] < x) lo = mid + 1u; else hi = mid; }
    return lo;
}
__global__ void agx_k_idm_bounds(agx_unitig_region_args R, agx_idmap_args M) {
    if (blockIdx.x || threadIdx.x > 1u) return;
    const agx_u32 n = M.n_ids > M.n_pos ? M.n_ids - M.n_pos : 0u;
    M.bounds[threadIdx.x] = idm_lower(M.side_xpos, n, threadIdx.x ? R.pos_lo + R.n_win : R.pos_lo);
}
struct idm_entry { agx_u32 seg, rank; };
// the entry of window id i (i < n_main + n_side); seg NONE: not in the export
__device__ __forceinline__ idm_entry idm_entry_of(const agx_unitig_region_args &R, const agx_idmap_args &M, agx_u32 i) {
    idm_entry e{AGX_NONE, 0u};
    const agx_u32 a = i < M.n_main ? R.pos_lo + i : M.n_pos + M.side_lo + (i - M.n_main);
    if (a >= M.n_ids) return e;
    const agx_u32 slot = M.a_nid[a];
    if (slot >= R.pool_cap) return e;                    // NONE: a main id without a node
    const agx_u32 l = ut_locals{R}.in_export(slot);
    if (l == AGX_NONE) return e;                         // dead at this coverage
    const agx_u32 X = R.U.pos_of[l];
    if (X != (i < M.n_main ? a : M.side_xpos[a - M.n_pos])) { atomicOr(R.U.err, 8u); return e; }      // (the id's position is its node's: main ids are positions)
    e.seg = R.U.indeg[l]; e.rank = R.U.osucc[l];
    return e;
}
__device__ __forceinline__ bool idm_continues(const idm_entry &p, const idm_entry &e) { return p.seg != AGX_NONE && p.seg == e.seg && p.rank + 1u == e.rank; }
__global__ void __launch_bounds__(256) agx_k_idm_flags(agx_unitig_region_args R, agx_idmap_args M) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, n = M.n_main + M.n_side;
    const bool in = i < n;
    idm_entry e{AGX_NONE, 0u};
    if (in) e = idm_entry_of(R, M, i);
    idm_entry p;
    p.seg = __shfl_up(e.seg, 1, 64); p.rank = __shfl_up(e.rank, 1, 64);
    if (lane == 0) { p.seg = AGX_NONE; p.rank = 0u; if (in && i > 0) p = idm_entry_of(R, M, i - 1u); }
    if (i == M.n_main) p.seg = AGX_NONE;                 // a run never holds a main id and a side id
    if (i <= n) M.flag[i] = in && e.seg != AGX_NONE && !idm_continues(p, e) ? 1u : 0u;      // (entry n: the scan's closing zero)
}
__global__ void __launch_bounds__(256) agx_k_idm_runs(agx_unitig_region_args R, agx_idmap_args M) {
    const agx_u32 i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, n = M.n_main + M.n_side;
    const bool in = i < n;
    idm_entry e{AGX_NONE, 0u};
    if (in) e = idm_entry_of(R, M, i);
    idm_entry s;
    s.seg = __shfl_down(e.seg, 1, 64); s.rank = __shfl_down(e.rank, 1, 64);
    if (lane == 63u) { s.seg = AGX_NONE; s.rank = 0u; if (i + 1u < n) s = idm_entry_of(R, M, i + 1u); }
    if (!in || e.seg == AGX_NONE) return;
    if (i + 1u >= n || i + 1u == M.n_main) s.seg = AGX_NONE;
    const agx_u32 a = i < M.n_main ? R.pos_lo + i : M.n_pos + M.side_lo + (i - M.n_main);
    const agx_u32 r = M.foff[i + 1u] - 1u;               // starts at or in front of i, less one (an id that is present lies behind a start)
    if (r >= M.run_cap) { atomicOr(R.U.err, 8u); return; }
    if (M.flag[i]) { M.r_first[r] = a; M.r_seg[r] = e.seg; M.r_rank[r] = e.rank; }
    if (!idm_continues(e, s)) M.r_last[r] = a;
}

inline dim3 ut_grid(agx_u32 n) { return dim3((n + 255u) / 256u); }

}  // namespace

extern "C" void agx_launch_unitig_region_count(const agx_unitig_region_args *R, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_utr_count, ut_grid(R->n_win + 1u), dim3(256), 0, st, *R);
    agx_launch_exclusive_scan(R->cntw, R->offw, R->n_win, R->U.scan_tmp, st);
}

extern "C" void agx_launch_idmap_bounds(const agx_unitig_region_args *R, const agx_idmap_args *M, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_idm_bounds, dim3(1), dim3(64), 0, st, *R, *M);
}
extern "C" void agx_launch_idmap_flags(const agx_unitig_region_args *R, const agx_idmap_args *M, hipStream_t st) {
    const agx_u32 n = M->n_main + M->n_side;
    hipLaunchKernelGGL(agx_k_idm_flags, ut_grid(n + 1u), dim3(256), 0, st, *R, *M);
    agx_launch_exclusive_scan(M->flag, M->foff, n, M->scan_tmp, st);
}
extern "C" void agx_launch_idmap_runs(const agx_unitig_region_args *R, const agx_idmap_args *M, hipStream_t st) {
    const agx_u32 n = M->n_main + M->n_side;
    if (n && M->run_cap) hipLaunchKernelGGL(agx_k_idm_runs, ut_grid(n), dim3(256), 0, st, *R, *M);
}

extern "C" void agx_launch_unitig_region_phase1(const agx_unitig_region_args *R, hipStream_t st) {
    const agx_u32 n = R->U.pool_cap, ngrp = R->U.n_pos;
    if (!n) return;
    hipLaunchKernelGGL(agx_k_utr_compact, ut_grid(R->n_win), dim3(256), 0, st, *R);
    hipLaunchKernelGGL(agx_k_utr_degrees, ut_grid(n), dim3(256), 0, st, *R);
    if (R->U.n_ovf) hipLaunchKernelGGL(agx_k_utr_ovf, ut_grid(R->U.n_ovf), dim3(256), 0, st, *R);
    hipLaunchKernelGGL(agx_k_utr_internal, ut_grid(n), dim3(256), 0, st, *R);
    hipLaunchKernelGGL(agx_k_utr_group_count, ut_grid(ngrp * 64u), dim3(256), 0, st, *R);
    agx_launch_exclusive_scan(R->U.wcnt, R->U.woff, ngrp, R->U.scan_tmp, st);
    agx_launch_exclusive_scan(R->U.hcnt, R->U.hoff, ngrp, R->U.scan_tmp, st);
    hipLaunchKernelGGL(agx_k_utr_pieces, ut_grid(ngrp * 64u), dim3(256), 0, st, *R);
}

extern "C" void agx_launch_unitig_phase1(const agx_unitig_args *A, hipStream_t st) {
    if (A->n_pos) {
        hipLaunchKernelGGL(agx_k_ut_pos, ut_grid(A->n_pos), dim3(256), 0, st, *A);
        hipLaunchKernelGGL(agx_k_ut_degrees, ut_grid(A->n_pos), dim3(256), 0, st, *A);
    }
    if (A->n_ovf) hipLaunchKernelGGL(agx_k_ut_ovf, ut_grid(A->n_ovf), dim3(256), 0, st, *A);
    if (A->n_pos) hipLaunchKernelGGL(agx_k_ut_internal, ut_grid(A->n_pos), dim3(256), 0, st, *A);
    if (A->pool_cap) {
        const agx_u32 nwin = (A->pool_cap + 63u) / 64u;
        hipLaunchKernelGGL(agx_k_ut_piece_count, ut_grid(nwin * 64u), dim3(256), 0, st, *A);
        agx_launch_exclusive_scan(A->wcnt, A->woff, nwin, A->scan_tmp, st);
        hipLaunchKernelGGL(agx_k_ut_pieces, ut_grid(nwin * 64u), dim3(256), 0, st, *A);
    }
}

// phases 2 and 3 of either form.  R: the region export whose local view A is (A == &R->U, with its pieces: the host has refused a window without any); nullptr: the whole export
extern "C" void agx_launch_unitig_phase2(const agx_unitig_args *A, const agx_unitig_region_args *R, agx_u32 rounds, hipStream_t st) {
    const agx_u32 np = A->piece_cap;
    if (np) {
        hipLaunchKernelGGL(agx_k_ut_jump_init, ut_grid(np), dim3(256), 0, st, *A, np);
        hipLaunchKernelGGL(agx_k_ut_jump_link, ut_grid(np), dim3(256), 0, st, *A, np);
        for (agx_u32 r = 0; r < rounds; r++) hipLaunchKernelGGL(agx_k_ut_jump, ut_grid(np), dim3(256), 0, st, *A, np, r);
    }
    if (R) {          // (heads were counted per 64-id group with the pieces; A->n_pos is the groups)
        if (np) hipLaunchKernelGGL(agx_k_utr_head_assign, ut_grid(A->n_pos * 64u), dim3(256), 0, st, *R, np);
    } else if (A->n_pos) {
        hipLaunchKernelGGL(agx_k_ut_head_count, ut_grid(A->n_pos), dim3(256), 0, st, *A);
        agx_launch_exclusive_scan(A->hcnt, A->hoff, A->n_pos, A->scan_tmp, st);
        hipLaunchKernelGGL(agx_k_ut_head_assign, ut_grid(A->n_pos), dim3(256), 0, st, *A, np);
    }
    if (np) {
        if (R) hipLaunchKernelGGL(agx_k_utr_rank, ut_grid(A->n_pos * 64u), dim3(256), 0, st, *R, np, rounds & 1u);
        else hipLaunchKernelGGL(agx_k_ut_rank, ut_grid((A->pool_cap + 63u) / 64u * 64u), dim3(256), 0, st, *A, np, rounds & 1u);
    }
    agx_launch_exclusive_scan(A->s_len, A->s_off, np, A->scan_tmp, st);          // (the region's s_off and l_off lie over the pointer jumping's arrays, which the rank kernel was the last to read)
    agx_launch_exclusive_scan(A->s_links, A->l_off, np, A->scan_tmp, st);
}

extern "C" void agx_launch_unitig_phase3(const agx_unitig_args *A, const agx_unitig_region_args *R, hipStream_t st) {
    if (R) { if (A->pool_cap) hipLaunchKernelGGL(agx_k_utr_emit, ut_grid(A->pool_cap), dim3(256), 0, st, *R); }
    else if (A->n_pos) hipLaunchKernelGGL(agx_k_ut_emit, ut_grid(A->n_pos), dim3(256), 0, st, *A);
    if (A->n_ovf) {
        if (R) hipLaunchKernelGGL(agx_k_utr_links_ovf, ut_grid(A->n_ovf), dim3(256), 0, st, *R);
        else hipLaunchKernelGGL(agx_k_ut_links_ovf, ut_grid(A->n_ovf), dim3(256), 0, st, *A);
    }
    if (A->piece_cap) hipLaunchKernelGGL(agx_k_ut_links_sort, ut_grid(A->piece_cap), dim3(256), 0, st, *A);
}

extern "C" void agx_launch_unitig_link_support(const agx_unitig_region_args *R, const agx_u8 *n_flags, const agx_u32 *e_cnt, const agx_u32 *ovf_cnt, agx_u32 *l_sup, hipStream_t st) {
    if (R->U.pool_cap && R->U.link_cap) hipLaunchKernelGGL(agx_k_utr_link_support, ut_grid(R->U.pool_cap), dim3(256), 0, st, *R, n_flags, e_cnt, ovf_cnt, l_sup);
}

extern "C" void agx_launch_unitig_totals(const agx_unitig_args *A, agx_u32 *tot, hipStream_t st) {
    hipLaunchKernelGGL(agx_k_ut_totals, dim3(1), dim3(64), 0, st, *A, tot);
}
