// agx_kargs.h — kernel argument blocks and launcher prototypes shared by agx_kernels.hip and agx_engine.cpp.
#pragma once
#include <hip/hip_runtime_api.h>
#include "agx_core.h"

struct agx_prep_args {
    const agx_whit *whits; const agx_wside *sides;      // [n_hits] wire records in SAM file order: a hit's number is its place in the file, the order the tile lists are sorted into
    const agx_run *runs; agx_dhit *dhit; agx_u32 n_hits, k, n_pos;      // dhit[i]: the derived record of the i-th hit IN TILE ORDER (hit perm[i])
    agx_u32 *tile_cnt;        // [n_tiles] number of hits overlapping each tile
    agx_u32 *err;             // bit 0: same-strand mates; bit 1: alignment beyond the unit sequence; bit 2: the order the staging made is not the order of the hits' first tiles
    // r05: the hits are walked in the order of their first tile (perm: stage_order; tile_first[t] = hits in front of tile t's own in that order), so a tile's list is a
    // filter over a window of the order (agx_k_tile_fill).  ckey[i] = the last tile hit i reaches (NONE: dropped, or LONG — it spans `lookback` tiles or more and is
    // listed in long_list instead; more than AGX_LONG_MAX of those: every list of the unit is made by scatter, agx_k_bin_fill + agx_k_tile_sort)
    const agx_u32 *perm, *tile_first; agx_u32 *ckey; agx_u32 lookback; agx_u32 *long_list, *long_count;
    // r06, tile-ordered upload (tiled != 0): whits[i] IS the i-th hit of the tile order — its `row` field carries the hit's number, its left-mate row is row i, AGX_WF_DUP says
    // what the file neighbours would have said — and perm_out[i] = that number is written here for the tile lists (4 bytes per hit less to upload, no gather of wire records)
    agx_u32 tiled; agx_u32 *perm_out;
};

// the fallback (more than AGX_LONG_MAX long hits): every hit takes its places in dense lists from a counter per tile
struct agx_bin_args { const agx_dhit *dhit; agx_u32 n_hits; const agx_u32 *tile_off; agx_u32 *cursor; agx_u32 *unsorted; agx_u32 cap;   // cap: entries the lists can hold
                      const agx_u32 *long_count; };

struct agx_node_kargs {
    agx_sweep_args S;
    agx_u32 tile_lo, tile_hi;  // pass 0 sweeps tiles [tile_lo, tile_hi): a unit's first build sweeps a window of tiles as soon as its read rows have landed (r06)
    agx_u32 *pool_cnt;         // node ids handed out per region (counter r at pool_cnt[r * AGX_REGION_PAD]); keeps counting past the slice's end
    const agx_u32 *region_off; // [regions + 1] first node id of every region's slice of the pool
    agx_u32 spill_lo; agx_u32 *spill_cnt;   // ids [spill_lo, pool_cap) behind the slices, for regions whose slice is full (one counter)
    agx_u32 *mid_count; agx_u32 *mid_list;   // tiles whose buckets did not fit pass 0's
    agx_u32 *big_count; agx_u32 *big_list;   // tiles whose buckets did not fit pass 1's either
    agx_u32 fallback_queued;   // the two fallback passes are queued behind the main pass (a unit's builds start without them: most units never overflow a bucket)
    agx_u32 *status;           // bit 3: a tile overflowed the main pass and no fallback pass is queued; bit 0: a region's slice of the node pool exhausted; bit 1: bucket overflow in the global-scratch pass; bit 2: tile lists too small;
                               // bit 4 (set by agx_k_tile_fill, read by the main pass): the tile lists were not made
    agx_u32 list_cap;          // capacity of the tile lists: a tile whose list ends beyond it is skipped (the host re-runs with larger lists)
    const agx_u32 *big_n;      // passes 1 and 2: number of tiles in mid_list / big_list, read on the device (no host round trip)
    const agx_u32 *mid_n;
    agx_u32 *scratch;          // fallback pass: one [AGX_NF*AGX_MAXV_BIG*64] bucket area per resident wavefront
    agx_u32 *huge_count; agx_u32 *huge_list; const agx_u32 *huge_n; agx_u32 *scratch_huge; agx_u32 huge_queued;   // pass 3 (AGX_MAXV_HUGE variants): tiles pass 2 gave up on
    agx_u32 *slow_list; agx_u32 *slow_count;   // the edge build's pass-B list: the sweep itself enters multi-variant positions with a position-skipping step
};

struct agx_edge_kargs {
    agx_sweep_args S; agx_edge_ovf *ovf; agx_u32 *ovf_count; agx_u32 ovf_cap; agx_u32 list_cap;
    agx_u32 *slow_list; agx_u32 *slow_count;   // positions that need the per-hit pass (device-side list)
    agx_u32 n_hits; const agx_u32 *jump_list; agx_u32 n_jump;      // pass J: the hits whose left mate has several runs (listed by the host's staging)
    const agx_u32 *abort;                      // the node sweeps' status word: non-zero = the node table is incomplete, do nothing
    const agx_u32 *big_list; const agx_u32 *big_n;   // tiles the fallback pass wrote (their edges are all pass A/B's)
};
// Edge support (agx_k_edge_support): one more pass over the tile lists of a converged build.  It reads the front of the build and the final node table and writes
// only the counters: e_cnt parallel to n_next, ovf_cnt parallel to the overflow list (n_ovf: its live entries), and per tile the events it saw and the contributions it made
// (summed on the host: one counter for all wavefronts would be one contended address).  unmatched: contributions that found no edge, and events that met an index outside the tables.
struct agx_support_kargs {
    agx_sweep_args S; const agx_edge_ovf *ovf; agx_u32 n_ovf, n_hits, list_cap;
    agx_u32 *e_cnt, *ovf_cnt;          // [pool_cap * AGX_MAXE], [ovf_cap]: zeroed by the caller
    agx_u32 *tile_events, *tile_adds;  // [n_tiles] each: written for every tile
    agx_u32 *unmatched;                // zeroed by the caller
    const agx_u32 *abort;              // the build's status word
};
// Edge reads (agx_k_edge_reads): the same pass over the tiles [tile_lo, tile_lo + n_tiles) of a CHUNK of the window, twice.  emit == 0: cnt[p] = the selected
// contributions of chunk position p = (tile - tile_lo) * 64 + lane (written for all 64 lanes of every tile of the chunk).  emit != 0: off is the exclusive scan of cnt, and
// the lane writes its contributions to recs[off[p] ..) as 16-byte records (src_pos, dst_pos, src_var | dst_var << 16, the hit's file number perm[place]); rec_cap: the total
// the host read.  Reads the front, the node table and the counters; writes only cnt / recs and the error word: bit 0 a contribution without an edge, an index outside the
// tables or a list entry without a hit; bit 1 the emit pass disagrees with the count.
struct agx_reads_kargs {
    agx_sweep_args S; agx_reads_tab T; const agx_u32 *perm; agx_u32 n_hits, list_cap;
    agx_u32 tile_lo, n_tiles, emit;
    agx_u32 *cnt, *off, *scan_tmp;     // [n_tiles * 64 + 1] each (the closing count is the host's zero), and the block sums of the multi-launch scan between the passes
    agx_u32 *recs; agx_u32 rec_cap;    // four words per record, 16-byte aligned
    agx_u32 *err;
    const agx_u32 *abort;              // the build's status word
};
// The counters of the edges an edge-reads call listed (agx_k_edge_reads_support): edge i is (sp[i], vars[i] & 0xFFFF) -> (dp[i], vars[i] >> 16); sup[i] = its support
// (agx_reads_counter), AGX_NONE where the node table holds no such edge or an index lies outside the tables.
struct agx_reads_sup_args {
    agx_reads_tab T; const agx_u32 *node_start; const agx_u16 *node_cnt; agx_u32 n_pos, pool_cap, n;
    agx_u32 *sp, *dp, *vars, *sup;     // [n] each
};
// Unitig export (agx_unitig.hip): reads the node table a build left in HBM, writes only its own scratch.  Slot arrays are [pool_cap], piece arrays
// [piece_cap], segment arrays [piece_cap + 1] (every unitig head is a piece start, so there are never more segments than pieces).
struct agx_unitig_args {
    const agx_u32 *node_start; const agx_u16 *node_cnt; const agx_u8 *n_flags; const agx_u8 *n_base; const agx_u32 *n_next; const int *n_counts; const char *ref;
    const agx_edge_ovf *ovf; agx_u32 n_ovf; agx_u32 n_pos, pool_cap;
    agx_u32 *err;                   // bit 0: an edge that does not lead to a later position; bit 1: a slot index outside the pool; bit 2: the piece lists disagree
    // per slot
    agx_u32 *pos_of;                // position of every used slot (NONE: not a node)
    agx_u32 *indeg;                 // alive in-degree (distinct predecessors), reused as the slot's segment once heads are known
    agx_u32 *outs;                  // alive successors among the four inline slots, then the whole alive out-degree
    agx_u32 *succ;                  // the last alive inline successor, reused as the piece id of piece starts
    agx_u32 *oout, *osucc;          // distinct alive successors on the overflow list / the last of them (osucc reused as the node's rank in its unitig)
    agx_u32 *nxt;                   // the internal edge out of the node, or NONE
    agx_u8 *haspred;                // 1: the node has an internal predecessor
    // overflow list
    unsigned long long *ovf_hash; agx_u32 hash_mask; agx_u8 *ovf_first;      // open-addressing set of (src, dst): ovf_first[i] = entry i is the first of its edge
    // pieces (runs of slot+1 internal edges inside a 64-slot window)
    agx_u32 piece_cap;
    agx_u32 *wcnt, *woff;  // [pool_cap / 64 + 1] pieces per 64-slot window and their exclusive scan (a piece's id: its window's offset + its rank there)
    agx_u32 *p_len, *p_next;                           // nodes, the piece its last node's internal edge enters (slot, then piece id)
    agx_u32 *anc[2], *off[2];                          // pointer jumping: ancestor piece and the nodes in between (ping-pong)
    agx_u32 *p_seg;                                    // segment of a head piece
    // heads and segments
    agx_u32 *hcnt, *hoff;                              // [n_pos + 1] heads per position, exclusive scan
    agx_u32 *s_len, *s_links, *s_hpos, *s_hvar, *s_last; unsigned long long *s_cov;
    agx_u32 *s_off, *l_off, *l_cur;                    // scans of s_len / s_links, cursor of each segment's links
    char *seq; agx_u32 seq_cap;
    agx_u32 *l_to; agx_u32 link_cap;
    agx_u32 *scan_tmp;                                 // the multi-launch scans' block sums (the export's scans run one after another on its stream)
};

// Region export (agx_unit_unitigs_region): the same definition on the nodes of positions [pos_lo, pos_lo + n_win) that are alive at the CALLER's coverage.  Those nodes get
// dense LOCAL ids in (position, variant) order and every later phase runs over local ids, so nothing here is sized by the unit but the reverse map, which is only ever
// touched at the window's slots.  U is the local view: U.pool_cap = kept nodes, U.n_pos = 64-id groups (hcnt / hoff are per group), U.pos_of[id] = the node's position, the
// other per-slot arrays of U are per local id and hold local ids; U.node_start, n_base, n_next, n_counts, ref and ovf are the unit's own (U.n_flags is not read: alive is
// nk_cid and the count against min_cov, never AGX_NF_DEAD).  The jumping, totals and link-sort kernels of the whole export run on U unchanged; the others share their steps with it (agx_unitig.hip: ut_locals).
struct agx_unitig_region_args {
    agx_unitig_args U;
    const agx_u32 *nk_cid; const agx_u16 *node_cnt; agx_u32 pos_lo, n_win, min_cov, pool_cap;      // pool_cap: the unit's node slots (bounds what the table names)
    agx_u32 *cntw, *offw;           // [n_win + 1] kept nodes per position, exclusive scan (offw[n_win] = kept nodes)
    agx_u32 *l_slot;                // [kept] slot of every local id
    agx_u32 *rmap;                  // [pool_cap] slot -> local id.  Never cleared: slot s is in the export iff rmap[s] < kept and l_slot[rmap[s]] == s, whatever an earlier export left here
};

// Id map of a region export (agx_unit_unitigs_mapped): the walk ids of the window are WINDOW IDS i in [0, n_main + n_side) — the main ids pos_lo + i, then the side ids
// n_pos + side_lo + (i - n_main) of the same positions (the side block is position-major, so they are one range; agx_k_idm_bounds finds it by two bisections of side_xpos).
// Entry of a window id: (segment, rank) of its node through a_nid -> rmap / l_slot -> the (segment, rank) the region's rank kernel left per local id (R.U.indeg, R.U.osucc),
// or NONE where the id has no node in the export.  A run starts at an id that is present and does not continue its predecessor's segment at rank + 1.
struct agx_idmap_args {
    const agx_u32 *a_nid, *side_xpos; agx_u32 n_pos, n_ids;      // the walk preparation's: node slot of every walk id, position of every side id
    agx_u32 n_main, side_lo, n_side;                             // the window's ids (side_lo, n_side: read back from `bounds`)
    agx_u32 *bounds;                                             // [2] side ids in front of pos_lo / in front of pos_lo + n_main
    agx_u32 *flag, *foff;                                        // [n_main + n_side + 1] run-start flags (closing zero) and their exclusive scan
    agx_u32 *scan_tmp;
    agx_u32 *r_first, *r_last, *r_seg, *r_rank; agx_u32 run_cap; // [run_cap] the runs
};

// Evidence under the walk's records (agx_evidence.hip, agx_unit_walk_evidence): one launch set per CHUNK of flat graph bases [lo, lo + n) (lo a multiple of 64).
// The record arrays are the whole table's and accumulate over the chunks; everything named c_ / flag / foff / iv_ is the chunk's, indexed by flat base - lo or by the
// chunk's interval number.
struct agx_evidence_args {
    agx_evidence_tab T;
    agx_u32 lo, n, min_depth, min_support, n_recs;
    unsigned long long *r_steps, *r_dsum;      // [n_recs] numbered steps, depth summed over the bases with a node
    unsigned long long *r_dmin, *r_smin;       // [n_recs] value << 32 | base offset of the smallest depth / step (all ones: none yet), one 64-bit atomicMin each
    agx_u32 *noedge;                           // steps between two nodes that the node table holds no edge for
    agx_u32 *c_depth, *c_step, *c_votes;       // [n] per base (c_votes: only when the tracks are wanted, else nullptr)
    agx_u32 *flag, *foff, *scan_tmp;           // [n + 1] interval-start flags (closing zero) and their exclusive scan
    agx_u32 iv_cap;                            // the chunk's intervals (read back from foff[n] before the runs kernel)
    agx_u32 *iv_rec, *iv_first, *iv_last, *iv_dmin, *iv_smin;      // [iv_cap]; the minima start as all ones
    agx_u32 *err;                              // bit 0: an interval number beyond iv_cap
};

// Pair span (agx_span.hip, agx_unit_pair_span): one launch set per SUB-WINDOW [lo, lo + n) of the call's window [win_lo, win_hi).  The mark pass goes over all
// hit records whatever the sub-window (it clamps every fragment to it); its counts are those of the call's window and are the same in every sub-window's pass.
struct agx_span_args {
    const agx_dhit *dhit; const agx_run *runs; agx_u32 n_hits, n_runs, n_pos;
    agx_u32 win_lo, win_hi;                    // the call's window: the fragments counted are those that meet it
    agx_u32 lo, n;                             // the sub-window
    agx_u32 *start, *end;                      // [n + 1] fragments that begin at (or in front of and reach) / end on each position; zeroed; start becomes span, end becomes cross
    agx_u32 *sc, *scan_tmp;                    // [n + 1] the scan of start[x] - end[x - 1], and the scan's block sums
    agx_u32 *part; agx_u32 n_part;             // [3 * n_part] per wavefront of the mark pass: fragments that meet the window, kept hits, kept hits outside the unit
};
#define AGX_SPAN_BLOCKS 1024u   // workgroups of the mark pass at most (its lanes stride over the hits): 4096 partials of three words

// Pair span under the walk's records (agx_unit_walk_span): one launch set per CHUNK of flat graph bases, §14's shape.  E is the evidence kernels' own argument struct with
// span in the place of depth (c_depth = the chunk's span, r_dsum / r_dmin the span sums and minima, min_depth = min_support = min_span, noedge = the steps that are not
// forward), so that agx_k_ev_runs serves the thin intervals unchanged.  span / cross are the whole unit's.  A JUMP is a step between positions x and y > x + 1: the gather
// flags it, the emit pass lists it behind the flags' scan, the host sorts and merges the list into ENTRIES (x, y) ascending, each with the flat bases that take it, and
// agx_k_sp_jumps counts per entry the fragments with f_lo <= x and y <= f_hi.
struct agx_walk_span_args {
    agx_evidence_args E;
    const agx_dhit *dhit; const agx_run *runs; agx_u32 n_hits, n_runs, n_pos;
    const agx_u32 *side_xpos;                  // [n_ids - n_pos] the position of every side id
    const agx_u32 *span, *cross;               // [n_pos]
    agx_u32 *c_pos;                            // [n] the position of every base of the chunk
    agx_u32 *jflag, *joff;                     // [n + 1] jump flags (closing zero) and their exclusive scan; the scan's block sums are E.scan_tmp
    agx_u32 *jt_x, *jt_y, *jt_base; agx_u32 jt_cap;      // [jt_cap] the chunk's jumps as the emit pass lists them: positions and flat base
    const agx_u32 *e_x, *e_y; agx_u32 *e_cnt; agx_u32 n_ent;      // [n_ent] the entries, sorted by (x, y), and their counters (zeroed)
    const agx_u32 *l_base, *l_ent; agx_u32 n_list;       // [n_list] every jump once more: its flat base and its entry
};

// Mate links (agx_links.hip, agx_unit_mate_links).  T is §14's flat stretch table (only its stretch arrays and n_ids are read here).  own and the per-record
// counters are the call's; the slot table, its flags and the compacted output are one PASS's: a pass inserts the links whose left record lies in [a_lo, a_hi).
struct agx_links_args {
    agx_evidence_tab T;
    const agx_dhit *dhit; const agx_run *runs; agx_u32 n_hits, n_runs, n_pos;
    const agx_u32 *side_xpos;                  // [n_ids - n_pos] the position of every side id
    agx_u32 *own;                              // [n_pos] the smallest record with a graph base on the position; NONE: nobody
    agx_u32 *rec; agx_u32 n_recs;              // [5 * n_recs] per record: inside, open to the left, open to the right, pairs of links out, pairs of links in
    agx_u32 *part; agx_u32 n_part;             // [6 * n_part] per wavefront of the pass: kept hits, kept hits outside the unit, unowned, inside, open, link pairs
    agx_u32 *spart; agx_u32 n_spart;           // [2 * n_spart] per wavefront of the shadow pass: shadowed graph bases, owned positions
    agx_u32 count;                             // the pass adds to rec and part (the call's first pass only)
    agx_u32 a_lo, a_hi, min_pairs;
    agx_u32 init_all;                          // agx_k_ln_init: own and rec too, not the slots alone
    unsigned long long *t_key, *t_len; agx_u32 *t_n, *t_lo_min, *t_lo_max, *t_hi_min, *t_hi_max;      // [slots] the table, a structure of arrays
    agx_u32 slots, log2_slots;                 // slots = 2^log2_slots >= 2
    agx_u32 *flag, *off, *scan_tmp;            // [slots + 1] the kept slots' flags (closing zero) and their exclusive scan, and the scan's block sums
    unsigned long long *o_key, *o_len; agx_u32 *o_n, *o_lo_min, *o_lo_max, *o_hi_min, *o_hi_max; agx_u32 out_cap;      // [out_cap] the kept slots, dense, in slot order
    agx_u32 *words;                            // 0: error bits (1: own names no record, 2: an emit beyond out_cap); 1: pairs that found no slot; 2: slots in use
};

// Bubbles (agx_bubbles.hip, agx_unit_bubbles): behind phase 3 of a region export, over the segment and link tables it left in the export's scratch
// (read only: s_* [n_segs], s_off / l_off [n_segs + 1], l_to [n_links], seq [n_bases], l_sup [n_links] with support).  Everything written is the call's own, carved from
// what the export no longer reads.  Per segment [n_segs + 1] (a closing zero each): flag (a bubble whose branch segments have max_nodes nodes at most), kcnt / bcnt (its
// branch rows / the bases of its branch segments, 0 when not flagged) and their exclusive scans boff / koff / baoff.  The table: bubble rows [bub_cap], branch rows
// [row_cap], bases [base_cap] — the three totals the host read.
struct agx_bubbles_args {
    const agx_u32 *s_hpos, *s_hvar, *s_last, *s_len, *s_off, *l_off, *l_to; const unsigned long long *s_cov; const char *seq; const agx_u32 *l_sup;
    agx_u32 n_segs, n_links, n_bases, max_nodes;
    agx_u32 *s_in;                                           // [n_segs] links that enter each segment (zeroed by the caller)
    agx_u32 *flag, *kcnt, *bcnt, *boff, *koff, *baoff, *scan_tmp;
    agx_u32 *part; agx_u32 n_part;                           // [8 * n_part] per wavefront of the class kernel: forks, bubbles, TIP, NESTED, SINKS_DIFFER, SINK_SHARED, the longest branch of a bubble, broken segments
    agx_u32 *tot;                                            // [8] the same, summed (the longest: the maximum)
    agx_u32 bub_cap, row_cap, base_cap;
    agx_u32 *b_spos, *b_svar, *b_slast, *b_tpos, *b_tvar, *b_broff;      // [bub_cap]
    agx_u32 *r_pos, *r_var, *r_nodes, *r_seqoff, *r_seg, *r_in, *r_out; unsigned long long *r_cov;      // [row_cap]; r_seg: the branch segment (NONE: direct); r_in / r_out: the two links' numbers, then (agx_k_bb_support) their support
    char *o_seq;                                             // [base_cap]
    agx_u32 *err;                                            // bit 4 (16): an index outside the tables or a store beyond a capacity
};

#define AGX_SLOW_WAVES 8192u  // wavefronts of the per-hit edge pass if the occupancy query fails (normally: as many as are resident at once)

extern "C" {
// one kernel that zeroes up to eight u32 ranges
struct agx_zero_args { agx_u32 *p[8]; agx_u32 n[8]; };
void agx_launch_zero(const agx_zero_args *, hipStream_t);
void agx_launch_cm_tables(const void *cnt_runs, const void *cnt_chunks, agx_u32 n_cnt_chunks, const agx_cmseg *segs, const void *seg_chunks, agx_u32 n_seg_chunks,
                           agx_u32 *cm_start, agx_cmkey *cm, agx_cmhead *head, agx_u32 n_pos, agx_u32 n_cm, hipStream_t);      // cm_start[n_pos + 1], cm, n_pos + 1 heads from the count runs and the conti-mer runs (agx_core.h: agx_cntrun, agx_chunk)
void agx_launch_expand_codes(const void *packed, void *vcodes, size_t n_bases16, const unsigned long long *other, size_t n_other, hipStream_t);      // 2-bit base classes (agx_pack_classes2) + the listed other bases -> agx_vote_code bytes; n_bases16 a multiple of 16
// the rows from their upload form (differences against the reference under each row's anchor hit, or the 2-bit classes: agx_core.h) -> agx_vote_code bytes, then the listed other bases.
// cnt: zeros up to the next multiple of 64 rows; anchor_bits: eight words readable behind any block's first anchor; wref: the packed reference, one 32-bit word of slack behind
// position n_pos + 15; stride <= AGX_ROW_MAXSTRIDE
void agx_launch_expand_rows(const void *whits, agx_u32 nh, const void *wsides, const void *wruns, const agx_u32 *anchor_bits, const agx_u32 *block_first, const agx_u8 *cnt, const agx_u32 *block_off,
                            const agx_u16 *units, const void *wref, void *vcodes, agx_u32 n_rows, agx_u32 stride, const unsigned long long *other, size_t n_other, hipStream_t);
void agx_launch_patch_codes(const unsigned long long *other, size_t n_other, void *vcodes, hipStream_t);      // the listed bases alone (indices into the whole vote-code array)
void agx_launch_expand_runs(const void *wruns, agx_run *runs, agx_u32 n_runs, hipStream_t);      // wire formats (agx_core.h) -> working arrays
// compact wire forms (agx_core.h) -> the wire records, once per upload.  The sides' scratch: their runs and the scan's output, n + 1 words each, then the scan's own words
void agx_launch_expand_hits(const agx_chit_block *blocks, const void *esc, const agx_u32 *ext, void *whits, agx_u32 nh, agx_u32 maxlen, hipStream_t);
inline size_t agx_side_scan_words(size_t n) { const size_t nb = (n + 1 + 4095) / 4096, nb2 = (nb + 4095) / 4096; return 2 * (n + 1) + 2 * (nb + 1) + 2 * (nb2 + 1); }
void agx_launch_expand_sides(const agx_u16 *counts, const agx_cside_esc *list, agx_u32 n_list, void *sides, agx_u32 n, agx_u32 first, agx_u32 *scan, hipStream_t);
void agx_launch_expand_ref(const void *packed, void *ref, size_t n_pos16, const void *refx, agx_u32 n_refx, hipStream_t);      // 2-bit reference bases + the stretches of other bytes -> letters; n_pos16 a multiple of 16
void agx_launch_hit_prep(const agx_prep_args *, hipStream_t);
// exclusive scan of in[0..n] (n+1 entries; in[n] is read, its value reaches no output) into out[0..n]; out[n] = total.  tmp: 2*(nb+1) + 2*(nb2+1) words, nb = ceil((n+1)/4096), nb2 = ceil(nb/4096)
void agx_launch_exclusive_scan(const agx_u32 *in, agx_u32 *out, agx_u32 n, agx_u32 *tmp, hipStream_t);
void agx_launch_exclusive_scan1(const agx_u32 *in, agx_u32 *out, agx_u32 n, unsigned long long *desc, hipStream_t);      // one launch; desc: ceil((n+1)/4096) zeroed words
void agx_launch_exclusive_scan1_capped(const agx_u32 *in, agx_u32 *out, agx_u32 n, unsigned long long *desc, agx_u32 grid_cap, hipStream_t);      // the same with at most grid_cap workgroups (0: the launcher's own grid; the test hooks)
agx_u32 agx_scan_grid_limit(agx_u32 grid_cap);      // the workgroups such a launch takes at most on the current device: min(grid_cap, what the device holds at once)
void agx_launch_bin_fill(const agx_bin_args *, hipStream_t);
// the tile lists as the sweeps read them (32-byte records in SAM order): agx_k_tile_fill from the window of the tile order, or — the fallback — agx_k_tile_sort from bin_fill's dense lists
struct agx_fill_args { const agx_u32 *tile_off, *tile_first, *perm, *ckey; const agx_dhit *dhit; const agx_run *runs; void *recs; agx_u32 *scratch /* = bin_fill's `unsorted` */;
                       agx_u32 n_tiles, cap, k, lookback; const agx_u32 *long_list, *long_count; agx_u32 *err;
                       agx_u32 *status; agx_u32 dense_queued; };      // status bit 4 (16): this unit needs the scatter fallback and it is not queued (dense_queued = 0): the build is repeated with it
void agx_launch_tile_fill(const agx_fill_args *, hipStream_t);
void agx_launch_tile_sort(const agx_fill_args *, hipStream_t);
void agx_launch_node_sweep(const agx_node_kargs *, hipStream_t);
void agx_launch_node_sweep_big(const agx_node_kargs *, hipStream_t);
void agx_launch_edge_sweep(const agx_edge_kargs *, hipStream_t);                   // pass A (lanes = positions)
void agx_launch_edge_jump(const agx_edge_kargs *, hipStream_t);    // pass J (lanes = hits: steps that skip positions)
void agx_launch_edge_slow(const agx_edge_kargs *, hipStream_t);           // pass B (lanes = hits of the slow positions pass A listed)
// walk preparation (agx_core.h): after the scan of the side counts the node sweep left behind: ids, records and overflow edges
// n_nodes / n_ovf are read from device memory (the node-pool and overflow counters), so no host round trip separates the sweeps
// from the walk preparation; the grids are sized by the capacities.
void agx_launch_copy_out(void *const *dst, const void *const *src, const size_t *bytes, int n, hipStream_t);      // HBM -> registered host memory, by a kernel
void agx_launch_fetch_records(const agx_compact_args *, agx_u32 first, agx_u32 stride, agx_u32 rows, agx_u32 width, agx_walknode *out, hipStream_t);
void agx_launch_compact(const agx_compact_args *, const agx_u32 *chain_end, agx_u32 n_chain_end, const agx_u32 *n_ovf_dev, agx_u32 ovf_cap, hipStream_t);
// reprune (agx_core.h): DEAD bits, side_pk and tile_side[0 .. n_tiles) of a built node table at A->coverage; the caller zeroes tile_side[n_tiles] and queues the walk preparation behind it
void agx_launch_reprune(const agx_reprune_args *, agx_u32 n_tiles, hipStream_t);
// special ids: bitmap, rank scan (desc: the one-launch scan; null: the three-launch one with scan_tmp), records; block 0 of the last kernel also leaves the
// totals the host reads: out[0..2] = *a, *b, sp_rank[n_words]; *sum = nodes handed out = the sum of the region counters
// r06: where a streamed download cuts the walk graph (agx_engine.cpp: begin_streamed_download): piece w holds main ids [64 * word[w], 64 * word[w + 1]) (the last one: up to n_pos)
// and the side ids of those positions.  The host needs, before it can queue the copies, the special ids in front of every cut (sparse-table ranks: sp_rank at the cut's word)
// and the side ids in front of it (tile_side_start at the cut's tile): block 0 of the build's last kernel leaves them next to the counters, cut_out[0 .. n] = ranks (entry n: all
// main ids), cut_out[AGX_DL_PIECES + 1 ..] = side ids.
#define AGX_DL_PIECES 16u
struct agx_cut_args { agx_u32 n; agx_u32 word[AGX_DL_PIECES + 1]; agx_u32 *cut_out; };
static_assert(AGX_TILE == 64, "a cut's word of the special-id bitmap (64 ids) is also a tile of the side-id prefix: agx_collect_block and stream_cuts count positions in 64s");
void agx_launch_special(const agx_compact_args *, agx_u32 n_words, agx_u32 *sp_rank, agx_u32 *scan_tmp, unsigned long long *desc,
                        agx_u32 *out, const agx_u32 *a, const agx_u32 *b, const agx_u32 *pool_cnt, agx_u32 regions, agx_u32 *sum, const agx_cut_args *cuts, hipStream_t);
#define AGX_MID_WAVES 3072u     // wavefronts of pass 1 (3 per SIMD fit its LDS buckets); they stride over the list of tiles pass 0 gave up on
#define AGX_BIG_WAVES 256u      // resident wavefronts of the global-scratch fallback pass
#define AGX_HUGE_WAVES 32u      // wavefronts of pass 3 (0.85 MB of scratch each)
// unitig export: phase 1 (degrees, internal edges, pieces; the host reads the piece count), phase 2 (piece ranks, heads, segments, link counts; the host reads the totals),
// phase 3 (bases and links, once the scans are in: the host sized seq / links from them).  The region export has a count in front (kept nodes per position of the window and
// their scan; the host reads the total) and a phase 1 of its own (local ids, degrees, internal edges, pieces and heads per 64-id group); phases 2 and 3 and the totals are
// launched on its local view, A = &R->U, with R beside it (R = nullptr: the whole export)
void agx_launch_unitig_phase1(const agx_unitig_args *, hipStream_t);
void agx_launch_unitig_region_count(const agx_unitig_region_args *, hipStream_t);
void agx_launch_unitig_region_phase1(const agx_unitig_region_args *, hipStream_t);
void agx_launch_unitig_phase2(const agx_unitig_args *A, const agx_unitig_region_args *R, agx_u32 rounds, hipStream_t);
void agx_launch_unitig_phase3(const agx_unitig_args *A, const agx_unitig_region_args *R, hipStream_t);
void agx_launch_unitig_totals(const agx_unitig_args *, agx_u32 *tot, hipStream_t);      // tot[0..3] = segments, bases, links, error word
// id map of a region export: bounds (queued beside the region's count: the host reads them with the kept nodes), flags + scan (behind phase 2: the host reads the run count
// with the totals), runs (beside phase 3)
void agx_launch_idmap_bounds(const agx_unitig_region_args *, const agx_idmap_args *, hipStream_t);
void agx_launch_idmap_flags(const agx_unitig_region_args *, const agx_idmap_args *, hipStream_t);
void agx_launch_idmap_runs(const agx_unitig_region_args *, const agx_idmap_args *, hipStream_t);
void agx_launch_node_sweep_huge(const agx_node_kargs *, hipStream_t);
void agx_launch_edge_support(const agx_support_kargs *, hipStream_t);
void agx_launch_edge_reads(const agx_reads_kargs *, hipStream_t);      // one pass (count or emit) over the chunk's tiles
void agx_launch_edge_reads_support(const agx_reads_sup_args *, hipStream_t);
// behind phase 3 of a region export: l_sup[i] = support of link i's edge, the last node of its source segment -> the head node of its target segment, overflow duplicates summed
// (n_flags: the unit's, for AGX_NF_EOVF — only such tails walk the overflow list, once per link)
void agx_launch_unitig_link_support(const agx_unitig_region_args *, const agx_u8 *n_flags, const agx_u32 *e_cnt, const agx_u32 *ovf_cnt, agx_u32 *l_sup, hipStream_t);
// evidence of one chunk: the gather with the record summaries, the per-base numbers, the interval-start flags and their scan (the host reads foff[n]); then, with iv_cap set
// and the interval minima filled with ones, the intervals
void agx_launch_evidence_gather(const agx_evidence_args *, hipStream_t);
void agx_launch_evidence_runs(const agx_evidence_args *, hipStream_t);
// pair span of one sub-window: the mark pass over all hits (start, end and part zeroed by the caller), the difference, its scan, and span / cross in place of start / end
agx_u32 agx_span_partials(agx_u32 n_hits);      // wavefronts of the mark pass = entries of `part` / 3
void agx_launch_pair_span(const agx_span_args *, hipStream_t);
// pair span under the records, one chunk: the gather with the jump flags and their scan (the host reads joff[n]); with jt_cap set the jump list; with the entries uploaded and
// their counters zeroed the count over all hits and the scatter to the bases' steps; then the record summaries, the interval-start flags and their scan (the host reads
// E.foff[n] and goes on with agx_launch_evidence_runs on E)
void agx_launch_walk_span_gather(const agx_walk_span_args *, hipStream_t);
void agx_launch_walk_span_emit(const agx_walk_span_args *, hipStream_t);
void agx_launch_walk_span_jumps(const agx_walk_span_args *, hipStream_t);
void agx_launch_walk_span_flags(const agx_walk_span_args *, hipStream_t);
// mate links: wavefronts of a strided pass over n items (entries of part / 6, of spart / 2); the init (own, rec and the slots, or the slots alone); own and the shadow
// count (own initialised); one pass over all hits into the initialised slots, the flags of the kept slots, their scan and the dense copy (the host reads words and off[slots])
agx_u32 agx_links_partials(agx_u32 n);
void agx_launch_links_init(const agx_links_args *, hipStream_t);
void agx_launch_links_own(const agx_links_args *, hipStream_t);
void agx_launch_links_pass(const agx_links_args *, hipStream_t);
// bubbles: wavefronts of the class kernel (entries of part / 8); the in-degrees, the classes with their totals and the three scans (s_in zeroed; the host reads tot and
// the scans' last entries); with the three capacities set the rows and their bases; with l_sup set the rows' support
agx_u32 agx_bubbles_partials(agx_u32 n_segs);
void agx_launch_bubbles_class(const agx_bubbles_args *, hipStream_t);
void agx_launch_bubbles_emit(const agx_bubbles_args *, hipStream_t);
}
