/* agx.h — C-ABI of libagx.so, the MI355X engine for AlignGraph's per-unit graph build + extend path.
 *
 * The reference (baoe/AlignGraph, one C++03 file "AG" = AlignGraph/AlignGraph.cpp) has no plugin or FFI
 * interface; the drop-in seam is the body of its unit loop (AG:4765-4783):
 *
 *     loadGenome(genome, u);  loadContigAlignment(genome, u);  loadReadAlignment(genome, k, iv, u, mrl);
 *     extendContigs(genome, coverage, k, u);  scaffoldContigs(genome, u);
 *
 * which reads tmp/_genome.u.fa, tmp/_contigs.fa, tmp/_contigs_genome.u.psl, tmp/_reads.fa and
 * tmp/_reads_genome.u.bowtie and writes tmp/_initial_contigs.u.fa, tmp/_pre_extended_contigs.u.fa and
 * tmp/_extended_contigs.u.fa.  agx_run_unit() replaces exactly those five calls (INTEGRATION.md shows the
 * three-line patch); the finer-grained entry points below split the same work at the packed-array boundary
 * so that a caller can keep inputs resident on the device and time host parsing, upload, kernels and the
 * walk separately.
 *
 * Plain C: pointers and sizes only, no C++ or torch types.  Every function returns AGX_OK (0) or a negative
 * AGX_E_* code; the message is available from agx_unit_error().  Nothing here ever exits the process or throws
 * across the boundary (the reference prints to stdout and exit(-1)s; INTEGRATION.md maps codes back to its
 * messages).  There is no CPU fallback: without a HIP device agx_unit_create() fails with AGX_E_NOGPU.
 *
 * Threading: an agx_unit is single-owner.  Distinct units may be driven concurrently, on one device or several.
 *
 * Device memory: ONE process per device is assumed.  The first unit of 8 GB or more makes a per-device region of AGX_REGION_PERCENT (default 85) per cent of the HBM
 * that is free at that moment and keeps it while anything lives in it (csrc/agx_mem.h: freed HBM stalls the next hipMalloc for seconds); a host that runs several
 * processes on one device sets the percentage per process, or AGX_NO_REGION=1 (every block then comes from hipMalloc or the cache of whole blocks).
 */
#ifndef AGX_H
#define AGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_OK 0
#define AGX_E_IO (-1)          /* "CANNOT OPEN FILE!"                                   AG:317, 356, 401, 849, 1274 */
#define AGX_E_FORMAT (-2)      /* "BROKEN BOWTIE FILE", "unknown character: c"           AG:1253, 267 */
#define AGX_E_UNSUPPORTED (-3) /* inputs the reference would index out of bounds on (DESIGN.md "Rejected inputs") */
#define AGX_E_ALIGNMENT (-4)   /* "BOWTIE ALIGNMENT ERROR" (mates on the same strand)    AG:1669 */
#define AGX_E_DEVICE (-5)      /* HIP runtime error */
#define AGX_E_ARG (-6)
#define AGX_E_OVERFLOW (-7)    /* more node variants at one position than the engine holds (AGX_MAXV_HUGE in agx_core.h: 1024; the reference's vector<KMer> is unbounded, AG:1375-1390) */
#define AGX_E_NOGPU (-8)

typedef struct agx_unit agx_unit;

/* Scalars of the unit loop: --kMer, --insertVariation, --coverage (AG:4701) and the compile-time BATCH (AG:37). */
typedef struct {
    uint32_t k;                /* default 5 */
    uint32_t insert_variation; /* default 50 */
    uint32_t coverage;         /* default 20 */
    uint32_t batch;            /* pairs per read batch; 0 = 1000000 (AG:37) */
    int32_t device;            /* HIP device ordinal */
    uint32_t flags;            /* AGX_FLAG_* */
} agx_params;

#define AGX_FLAG_KEEP_COUNTS 1u /* keep per-node coverage and base votes on the device for agx_unit_graph() */
#define AGX_FLAG_TIME_SECTIONS 4u /* time every section of a build (agx_stats ms_prep .. ms_compact); without it only ms_node_sweep is measured: an event
                                     record between two kernels costs the stream about as much as a small kernel */
#define AGX_FLAG_SPARSE_MIN  2u /* test hook: download node records of the side ids only, read all others one by one from the device */
#define AGX_FLAG_ONE_SHOT    8u /* the unit is uploaded ONCE after its inputs were handed over (the application's flow, agx_run_unit): once they are in HBM the
                                     staged input arrays are dead, and the download lands in that pinned memory instead of mapping and pinning 5 bytes per
                                     position of fresh memory per unit.  Another upload needs the inputs handed over again (agx_unit_load_files / push_pairs) */

#define AGX_FLAG_KEEP_PATHS 16u /* agx_unit_finish keeps the graph stretches of every written pre-extended record for agx_unit_walk_paths, and (with AGX_FLAG_KEEP_COUNTS) the
                                     unit's block reserves the scratch of agx_unit_unitigs_mapped.  The outputs of a finish are the same bytes with and without it */

#define AGX_FLAG_EDGE_SUPPORT 32u /* the unit's block also holds one counter per edge (four bytes per inline edge slot and per overflow entry) for agx_unit_edge_support and
                                     agx_unit_unitigs_support.  A build queues nothing for it: the counting runs on the first request after a build */

/* ---- packed inputs -------------------------------------------------------------------------------- */

/* n read bases from read index q sit on reference offsets t, t+1, ...  (Segment, AG:44-49) */
typedef struct { uint32_t q, t, n; } agx_run;

/* One (pair, hit) that passed the identity filter of loadReadAli (AG:1261), in SAM order. */
typedef struct {
    uint32_t slot1;         /* mate1's slot in the read-base blob; mate2 is slot1+1 */
    uint32_t pos1, pos2;    /* "simple" mates (one M run covering the whole read): reference offset of read index 0 */
    uint32_t runs1, runs2;  /* first run in the run pool (non-simple mates) */
    uint16_t nruns1, nruns2; /* 0 = simple */
    uint16_t len;           /* read length; mates are equal length (AG:3454) */
    uint8_t rev1, rev2;     /* SAM FLAG 0x10 of each mate */
    uint8_t back;           /* number of earlier kept hits of the same pair */
    uint8_t pad[3];         /* ignored */
} agx_hit;

/* ContiMer (AG:51-62) inside a unit: the chromosome id is always 0 */
typedef struct { uint32_t cid, coff, next_off, next_item; char nuc; char pad[3]; } agx_contimer;

typedef struct {
    const agx_hit *hits; uint64_t n_hits;
    const agx_run *runs; uint64_t n_runs;
    const char *bases;      /* read slot s occupies bases[s*stride .. s*stride+len) in reads-file orientation */
    uint32_t stride, n_slots;
} agx_pair_batch;

/* ---- outputs --------------------------------------------------------------------------------------- */

typedef struct {
    char *initial_contigs; size_t initial_len;   /* bytes of tmp/_initial_contigs.u.fa      (AG:1179-1216) */
    char *pre_extended;    size_t pre_len;       /* bytes of tmp/_pre_extended_contigs.u.fa (AG:2176-2189) */
    char *extended;        size_t extended_len;  /* bytes of tmp/_extended_contigs.u.fa     (AG:2451-2463) */
} agx_result;

typedef struct {
    uint64_t n_pos, n_ref, n_hits, n_runs, n_nodes, n_tiles, n_tile_entries, n_big_tiles, n_edge_overflow;
    uint64_t pairs_in_file, sam_line_pairs;
    double ms_parse, ms_thread, ms_upload, ms_prep, ms_bin, ms_node_sweep, ms_node_big, ms_edge_sweep, ms_compact, ms_download, ms_walk;
    uint32_t node_sweep_launches, edge_sweep_launches;
    uint64_t n_walk_ids, n_special, n_fetched, download_bytes;   /* walk graph: ids, node records downloaded, records fetched one by one, D2H bytes */
    double ms_edge_fast, ms_edge_slow;                           /* the two kernels of ms_edge_sweep: pass A (lanes = positions), pass B (lanes = hits) */
    uint64_t n_mid_tiles;                                        /* tiles swept again with wider LDS buckets (n_big_tiles: of those, again with global scratch) */
    double ms_build_span;                                        /* with AGX_FLAG_TIME_SECTIONS: device time from the first to the last command of the build (all kernels and the gaps between them) */
    double ms_stage;                                             /* packing the handed-over arrays into pinned upload buffers (agx_unit_stage) */
    double ms_upload_dev;                                        /* with AGX_FLAG_TIME_SECTIONS: device time of the unit's upload copies on the device's upload stream */
    uint64_t upload_bytes, device_bytes;                         /* bytes copied host -> HBM by the upload (AGX_WIRE_PLAIN=1: hit and side records as they are, not in their compact wire forms); HBM held by the unit */
    uint64_t pinned_bytes_cached, device_bytes_cached;           /* free blocks in the library's pinned-host and device caches (agx_pool_trim releases them) */
    uint64_t n_spilled;                                          /* node ids taken from the pool's spill area (regions whose slice was full) */
    uint32_t build_attempts, from_cache;                         /* build_attempts: 1 unless a capacity had to grow and the build was repeated; from_cache: the unit was
                                                                    loaded from its cache file (agx_unit_cache_build), not from the text files */
    uint32_t dense_lists, rows_by_reference;                     /* dense_lists: 0 = every tile's hit list came out of its window of the hits' tile order (agx_k_tile_fill); 1 = some hits
                                                                    span more tiles than the window looks back over (long deletions) and came through the list of long hits; 2 = more than
                                                                    1024 such hits: every list of the unit was made by scatter (agx_k_bin_fill + agx_k_tile_sort).
                                                                    rows_by_reference: read rows the upload sent as their differences from the reference under their first hit's
                                                                    alignment (AGX_ROW_DIFF, engine: stage_rows; 0: all rows crossed as 2-bit classes) */
    uint64_t n_edge_slow;                                        /* positions the edge build's pass B resolved hit by hit: multi-variant positions with a step elsewhere, listed by the
                                                                    node sweep, and the positions pass A found with several variants there or at x+1 */
    uint32_t reprune_attempts;                                   /* of the last agx_unit_reprune: 1 unless the sparse record table had to grow and the reprune was repeated */
    double ms_reprune;                                           /* host wall time of the last agx_unit_reprune, from entry to its counters being back */
    double ms_edge_support;                                      /* host wall time the last agx_unit_edge_support / agx_unit_unitigs_support spent making sure the edge counters are there: zeroing,
                                                                    the counting kernel and the wait for its totals on the first call after a build, next to nothing on later ones */
    uint64_t n_support_events;                                   /* events the counting saw (agx_edge_support::n_events); 0 before the first counting call after a build */
    double ms_walk_evidence;                                     /* host wall time of the last agx_unit_walk_evidence, from entry to its tables being in the caller's memory */
    double ms_edge_reads;                                        /* host wall time of the last agx_unit_edge_reads, from entry to its table being in the caller's memory; 0 before the first call */
    double ms_pair_span;                                         /* host wall time of the last agx_unit_pair_span, from entry to its table being in the caller's memory; 0 before the first call */
    double ms_walk_span;                                         /* the same of the last agx_unit_walk_span */
} agx_stats;

/* Node/edge tables in canonical numbering (position-major, variant order), for parity tests. malloc'd; free with agx_graph_free. */
typedef struct {
    uint32_t n_pos, n_nodes, n_edges;
    uint32_t *node_start;   /* [n_pos+1] */
    uint32_t *node_key;     /* [n_nodes*6] contigID, contigOffset, contigID0, contigOffset0, chromosomeID0, chromosomeOffset0 */
    int32_t *node_cnt;      /* [n_nodes*6] coverage, A, C, G, T, N   (needs AGX_FLAG_KEEP_COUNTS, else all -1) */
    uint32_t *node_slen;    /* [n_nodes] length of the stored k-mer string */
    uint32_t *edge_start;   /* [n_nodes+1] */
    uint32_t *edge_dst;     /* [n_edges] sorted per node */
} agx_graph;

/* A unit's pruned graph compacted into unitigs (maximal paths of internal edges: u -> v with one alive successor of u, one alive
 * predecessor of v), for GFA export.  Segments are in the order of their head nodes (position, then variant in agx_unit_graph's
 * order); links are the alive edges that are not internal, by (from, to) segment.  malloc'd; free with agx_unitigs_free. */
typedef struct {
    uint32_t n_segs, n_links;
    uint64_t n_bases;       /* = seq_off[n_segs] */
    uint32_t *head_pos;     /* [n_segs] position of the head node */
    uint32_t *head_var;     /* [n_segs] its variant index at that position */
    uint32_t *n_nodes;      /* [n_segs] nodes (= bases) of the segment */
    uint32_t *last_pos;     /* [n_segs] position of the last node */
    uint64_t *coverage;     /* [n_segs] sum of the nodes' coverage */
    uint64_t *seq_off;      /* [n_segs + 1] segment s is seq[seq_off[s] .. seq_off[s+1]) */
    char *seq;              /* [n_bases] one base per node: the consensus, or the reference base where the node has no votes */
    uint32_t *link_from, *link_to;   /* [n_links] segment indexes */
} agx_unitigs;

/* Edge support: for every edge of agx_unit_graph, in its numbering (edge_start / edge_dst are that call's arrays), the number of EVENTS that name it.  An event
 * is one step of one kept hit from an aligned position P to the next one N inside the unit — one call of the reference's updateKMer (AG:1353-1624) with a k2 half.  It names
 * every pair (s, d) of a variant s that one of its candidate keys at P resolves to and a variant d that one of its candidate keys at N resolves to, if the pair passes the
 * contig-consistency test of AG:1602-1615; each pair once per event.  Every edge has support >= 1, no event names a pair that is not an edge, and the numbers do not depend on
 * the coverage threshold.  n_events: the events; n_contributions: the sum of edge_cnt.  malloc'd; free with agx_edge_support_free. */
typedef struct { uint32_t n_nodes, n_edges; uint64_t n_events, n_contributions;
                 uint32_t *edge_start, *edge_dst, *edge_cnt; } agx_edge_support;

/* Edge reads: the hits behind the edges of a window.  Events, named edges and support are agx_edge_support's.  An edge (s, d) is SELECTED iff the position of
 * s lies in [pos_lo, pos_hi) and its support is <= max_support (0xFFFFFFFF: every edge whose source lies in the window; 0: none, every edge has support >= 1); the position of d
 * may lie outside the window.  The table holds every selected edge — as (src_pos, src_var) -> (dst_pos, dst_var), var the index among ALL of the position's variants, agx_unitigs'
 * head_var — ordered by (src_pos, src_var, dst_pos, dst_var), and for edge e its support and, in hit[hit_off[e] .. hit_off[e + 1]), the HIT NUMBER of every event that names it,
 * ascending.  A hit number is the hit's place in the order the hits were handed over: the i-th agx_hit of all agx_unit_push_pairs batches, counted from 0 — for the file
 * loaders the i-th (pair, hit) of tmp/_reads_genome.<u>.bowtie that passed the identity filter —, which is the index into agx_front's dhit in file order (perm[]).  One hit
 * names an edge in one event at most (a hit has one arrival per position, and an edge's source is one position), so the numbers of an edge are distinct and
 * hit_off[e + 1] - hit_off[e] == support[e].  The table does not depend on the coverage threshold or on a reprune.  malloc'd; free with agx_edge_reads_free. */
typedef struct { uint32_t n_edges; uint64_t n_hits;
                 uint32_t *src_pos, *src_var, *dst_pos, *dst_var, *support;   /* [n_edges] */
                 uint64_t *hit_off;                                           /* [n_edges + 1] */
                 uint32_t *hit; } agx_edge_reads;                             /* [n_hits] */

/* The id map of an export (agx_unit_unitigs_mapped): which walk ids have their node in the export, and where.  Runs are sorted by id_first; walk id a lies in run r iff
 * id_first[r] <= a <= id_last[r], and its node is then node number rank_first[r] + (a - id_first[r]) of segment seg[r].  Runs are maximal (no two neighbours could be merged)
 * and never hold both a main id (< n_pos) and a side id.  Ids without a node, and ids whose node lies outside the window or is dead at the export's coverage, are in no run.
 * malloc'd; free with agx_idmap_free. */
typedef struct {
    uint32_t n_runs, n_pos, n_ids;      /* n_pos, n_ids: the unit's positions and walk ids */
    uint32_t *id_first, *id_last, *seg, *rank_first;   /* [n_runs] */
} agx_idmap;

/* The graph stretches of the records of pre_extended (extdContigs1, AG:1954-2204; the records it writes, AG:2176-2189), kept by a finish of a unit created with
 * AGX_FLAG_KEEP_PATHS.  Record r is the r-th record of pre_extended (header number seqID = r); its stretches are st_off[r] .. st_off[r + 1).  A stretch is a run of
 * consecutive walk ids id_first .. id_last (inclusive) whose bases are the record's bases [base_off, base_off + id_last - id_first + 1).  joined = 1 iff the stretch starts
 * exactly where the previous stretch of the same record ended: the walk then went from the previous id_last to this id_first over an edge; 0 for a record's first
 * stretch and behind a conti-mer chain.  The bases of chains and the record's trailing k-mer belong to no stretch.  malloc'd; free with agx_walk_paths_free. */
typedef struct {
    uint32_t n_recs; uint64_t n_stretches;
    uint64_t *rec_len;         /* [n_recs] bases of each record */
    uint64_t *st_off;          /* [n_recs + 1] */
    uint32_t *id_first, *id_last; uint64_t *base_off; uint8_t *joined;   /* [n_stretches] */
} agx_walk_paths;

/* Evidence under the walk's records: the per-node coverage and votes and the per-edge support (§13) joined, on the device, to the bases of the records
 * of a stretch table w.  A GRAPH BASE is a base that lies in a stretch; base b of stretch s is walk id id_first[s] + (b - base_off[s]).  A STEP leaves a graph base toward
 * the next base of its stretch, or — from a stretch's last base — toward the first base of the next stretch of the record if that has joined = 1.  0xFFFFFFFF stands
 * for "no number" everywhere: a depth of an id without a node, a step that does not exist, has an end without a node, or names a pair the node table holds no edge for
 * (those are counted in n_steps_without_edge), and every step of a unit without AGX_FLAG_EDGE_SUPPORT.
 * Per record: graph bases, numbered steps, the depth summed over the bases with a node, the smallest depth and the smallest numbered step, each with the smallest base
 * offset that has it (value 0xFFFFFFFF, offset 0: none).  Weak intervals: maximal runs of weak bases of one record at consecutive base offsets, by (rec, first); a base
 * is weak iff it has no node, its depth is below min_depth, or its step has a number below min_support; iv_depth_min / iv_step_min: the smallest depth of a node / the
 * smallest numbered step in the interval.  Tracks (want_tracks): depth, votes (the largest of the node's five vote counters) and step per graph base of the records
 * [rec_lo, rec_hi) in stretch order; track_off has one entry per stretch of those records and a closing one: the stretch st_off[rec_lo] + i begins at entry track_off[i].
 * malloc'd; free with agx_walk_evidence_free. */
typedef struct { uint32_t n_recs, n_intervals; uint64_t n_graph_bases, n_steps, n_steps_without_edge;
                 /* [n_recs] */ uint64_t *rec_graph_bases, *rec_steps, *rec_depth_sum; uint32_t *rec_depth_min, *rec_depth_min_at, *rec_step_min, *rec_step_min_at;
                 /* [n_intervals] */ uint32_t *iv_rec, *iv_first, *iv_last, *iv_depth_min, *iv_step_min;
                 /* tracks, want_tracks only */ uint32_t rec_lo, rec_hi; uint64_t n_track; uint64_t *track_off; uint32_t *depth, *votes, *step; } agx_walk_evidence;

/* The walk graph: what the walk preparation (csrc/agx_core.h "walk preparation") leaves on the device and the download carries to the host walk (GraphView, csrc/agx_host.h).
 * Walk ids [0, n_pos) are the first alive variant of each position, [n_pos, n_ids) the further ones.  malloc'd; free with agx_walk_graph_free. */
typedef struct { uint32_t next[4]; uint32_t off0, xpos, sref_slot, sref_qlen; } agx_walk_rec;   /* successors (walk ids, 0xFFFFFFFF = none), mate offset, position, k-mer string (length: bits 16..30 of sref_qlen) */
typedef struct { uint32_t str_off, len, end_pos; } agx_walk_hop;                                  /* leave the k-mer graph: append chain_str[str_off, str_off + len), land on end_pos; len 0 = no hop */
typedef struct {
    uint32_t want_all_node;    /* IN: non-zero = also fill all_node (set it in a zeroed struct before the call) */
    uint32_t n_pos, n_ids, n_special, n_ovf;
    uint64_t n_chain_str;
    uint8_t *meta;             /* [n_ids] AGX_WM_* bits: 1 forced step to id + 1, 2 on a contig, 4 side ids at the position, 8 a variant at the position, 128 no node */
    char *str;                 /* [n_ids] the base a node emits */
    uint32_t *side_xpos;       /* [n_ids - n_pos] position of each side id */
    uint64_t *sp_bits;         /* [n_ids / 64 + 1] special-id bitmap */
    uint32_t *sp_rank;         /* [n_ids / 64 + 1] special ids before each 64-id word */
    agx_walk_rec *sp_node;  /* [n_special] records of the special ids, id order */
    agx_walk_hop *sp_hop;      /* [n_special] hop entry of each special id's position */
    uint32_t *ovf;             /* [n_ovf * 2] overflow edges (source, target) in walk ids; 0xFFFFFFFF pairs and duplicates are to be ignored */
    char *chain_str;           /* [n_chain_str] the unit's conti-mer chain bases (agx_walk_hop::str_off points in here) */
    agx_walk_rec *all_node; /* [n_ids] (want_all_node) every id's record, read through the path the walk fetches single records by */
} agx_walk_graph;

/* The front of a build: what the device holds in front of the node sweep after the last converged attempt of agx_unit_build — the arrays the first build expands
 * out of their upload forms (whichever forms the unit used: the contents are the same), the derived hit records and the tile lists.  Hits are in the DEVICE's order
 * (the order of their first tile); perm[i] is the file number of the hit at place i.  malloc'd; free with agx_front_free. */
typedef struct {
    uint32_t n_pos, n_hits, n_runs, n_cm, n_tiles, stride, n_rows;   /* n_rows: rows of vcodes (tile-ordered upload: one per hit; else one per staged read row) */
    uint32_t lookback;         /* tiles a list's window of the tile order looks back over */
    uint32_t n_entries;        /* = tile_off[n_tiles] */
    uint32_t long_count, n_long;   /* hits that span lookback tiles or more; n_long = min(long_count, 1024) of them are listed */
    uint32_t w_err, w_status;  /* the build's error and status words (0, 0: nothing went wrong; status bits that made an earlier attempt repeat are gone) */
    uint32_t tiled, rows_diffed, ref_packed, dense_queued, swept_windows;   /* the forms the unit used: tile-ordered upload, read rows as differences from the reference, unit sequence as 2 bits
                                                                               per base, the scatter fallback of the tile lists queued, windows the last attempt's node sweep ran in */
    char *ref;                 /* [n_pos] */
    uint8_t *vcodes;           /* [n_rows * stride] vote codes; a row's bytes from the read's length up to the stride are class-0 codes, bytes behind the last row are not copied */
    agx_run *runs;             /* [n_runs] */
    uint32_t *cm_start;        /* [n_pos + 1] */
    uint32_t *cm;              /* [n_cm * 2] cid, coff */
    uint32_t *cm_head;         /* [(n_pos + 1) * 4] cid, coff, n, start; entry n_pos: "no position" */
    uint32_t *dhit;            /* [n_hits * 10] the derived records as ten words: a_t0, b_t0, a_runs, b_runs, a_slot, len | jstar << 16, a_nruns | b_nruns << 16, flags, x_lo, x_hi */
    uint32_t *perm;            /* [n_hits] */
    uint32_t *tile_first;      /* [n_tiles + 1] places in front of each tile's own hits */
    uint32_t *ckey;            /* [n_hits] last tile of the hit at place i; 0xFFFFFFFF for skipped and long hits */
    uint32_t *tile_cnt;        /* [n_tiles + 1] the histogram (entry n_tiles: 0) */
    uint32_t *tile_off;        /* [n_tiles + 1] its exclusive prefix sum */
    uint32_t *tile_recs;       /* [n_entries * 8] qoff1, boff1, qoff2, boff2, slot, len | jstar << 16, geo, hit (place in the device's order) */
    uint32_t *long_list;       /* [n_long] places of the long hits, in the order the atomics gave */
} agx_front;

/* ---- entry points ------------------------------------------------------------------------------------ */

const char *agx_version(void);
int agx_device_count(void);                                   /* HIP devices visible; 0 when there is no GPU */
int agx_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);   /* HBM of one device (hipMemGetInfo) */
int agx_selftest_scan(int device, uint32_t n, uint32_t seed);   /* test hook: the build's one-launch prefix scan over n pseudo-random counts against a host scan; AGX_OK or AGX_E_DEVICE */

/* Test hooks of the primitives under every build and export: the caller's arrays through the library's own launchers.  Every device array is followed
   (agx_test_zero: also preceded) by AGX_TEST_GUARD words of 0xA5 bytes that come back with it.  AGX_OK, AGX_E_ARG or AGX_E_DEVICE.
   agx_test_scan: the exclusive scan of in[0 .. n] (n + 1 words; in[n] is read, no output may depend on it) into out[0 .. n].
     form 0: the multi-launch scan; tmp[2 (nb + 1) + 2 (nb2 + 1) + guard] comes back, nb = ceil((n + 1) / 4096), nb2 = ceil(nb / 4096); grid_cap = seeded = 0.
     form 1: the one-launch scan; desc[nb + guard] comes back (zeroed before the launch).  grid_cap: 0, or the most workgroups the launch may take (never more than the
             launcher's own grid); *grid_limit = the limit that held.  seeded: every desc[b] holds the aggregate flag and block b's own sum before the launch.
     streams: 1, or 2 (grid_cap = 0): the scan twice at once on two streams; out, desc and tmp then hold the second run behind the first. */
#define AGX_TEST_GUARD 64
int agx_test_scan(int device, int form, const uint32_t *in, uint32_t n, uint32_t *out /* [streams][n + 1 + guard] */, uint32_t grid_cap, int seeded, int streams,
                  uint64_t *desc, uint32_t *tmp, uint32_t *grid_limit);
/* agx_k_zero over eight arrays of len[0 .. 7] words; words: the eight arrays one after the other, each as guard | len[s] | guard */
int agx_test_zero(int device, const uint32_t *len, uint32_t *words);
/* agx_launch_copy_out of n_seg (1 .. 16) segments from device memory to registered host memory.  src: the segments one after the other, each padded to a multiple of
   16 bytes; dst: what the host buffer holds afterwards, each segment as (padded bytes | guard) */
int agx_test_copy_out(int device, int n_seg, const uint64_t *bytes, const uint8_t *src, uint8_t *dst);
/* Test hook of the on-request calls (agx_unit_unitigs and everything behind it in this file): overwrites what such a call must not trust, as a process that has answered
   other questions about other units leaves it.  what & 1: every byte of the export's scratch, taken as any export takes it (agx_unit_hbm_needed and device_bytes are then
   what they are after an export); what & 2: the edge counters of a unit with AGX_FLAG_EDGE_SUPPORT, unless they hold the last build's counts — valid counters are state
   and stay.  pattern 0: bytes 0x00; 1: 0xFF; 2: 0xA5; 3: 32-bit words of a xorshift of seed, uploaded.  Memsets and copies on a stream of the call's own, waited for; no
   kernel; nothing a build, walk or download reads is touched.  The preconditions of agx_unit_unitigs (AGX_E_ARG otherwise, also for other bits of `what` or pattern > 3,
   and nothing is written). */
int agx_test_poison(agx_unit *u, uint32_t what, uint32_t pattern, uint64_t seed);

int agx_unit_create(const agx_params *p, agx_unit **out);
void agx_unit_destroy(agx_unit *u);
const char *agx_unit_error(const agx_unit *u);

/* Packed-array boundary.  Pointers are borrowed for the call; the unit keeps its own copy. */
int agx_unit_set_reference(agx_unit *u, const char *bases, uint32_t n);                       /* replaces loadGenome, AG:287-320 */
int agx_unit_set_contig_threads(agx_unit *u, const char *appended, uint32_t n_appended,      /* result of updateGenomeWithContig, AG:884-1217 */
                                const uint32_t *cm_start, const agx_contimer *cm, uint32_t n_cm,
                                const char *initial_contigs, size_t initial_len);
int agx_unit_push_pairs(agx_unit *u, const agx_pair_batch *b);                                /* result of loadSeq + loadReadAli, AG:361-404, 1233-1277 */

/* Host loaders: the reference's own text files -> the three calls above. */
int agx_unit_load_files(agx_unit *u, const char *tmp_dir, int unit);

/* tmp/_reads.fa is the same file for every unit of a run, and the reference reads all of it for each unit (loadSeq under
 * loadReadAlignment, AG:1880).  An agx_reads maps it once and indexes its records; the _shared loaders then touch only the reads a
 * unit's own alignments name.  Immutable once opened: any number of host threads may load units from one agx_reads. */
typedef struct agx_reads agx_reads;
int agx_reads_open(const char *reads_fa, agx_reads **out, char *err, size_t err_len);
void agx_reads_close(agx_reads *reads);
int agx_unit_load_files_shared(agx_unit *u, const char *tmp_dir, int unit, const agx_reads *reads);   /* reads == NULL: same as agx_unit_load_files */

/* The binary cache of a unit's parsed inputs: tmp_dir/_agx_unit.<unit>.bin holds the unit's staged arrays, made from the
 * five text files once — AlignGraph_amd does it where the reference distributes the alignments (AG:3545-3579).  agx_unit_load_files* take
 * the cache instead of the text whenever it is current (same BATCH, the text files unchanged in size and modification time; AGX_NO_CACHE=1 in
 * the environment turns that off).  p: only batch and device matter. */
int agx_unit_cache_build(const agx_params *p, const char *tmp_dir, int unit, const agx_reads *reads, char *err, size_t err_len);
int agx_unit_cache_save(agx_unit *u, const char *tmp_dir, int unit);   /* the same file from a unit that agx_unit_load_files has just loaded from the text of (tmp_dir, unit) */

int agx_unit_stage(agx_unit *u);                 /* packs what was handed over into pinned upload buffers (read bases as 4-bit classes); done by agx_unit_load_files,
                                                    implied by agx_unit_upload after agx_unit_push_pairs */
int agx_unit_hbm_needed(agx_unit *u, uint64_t *bytes);   /* the HBM block agx_unit_upload will take for this (loaded) unit at its first-guess capacities: what a caller that shares a
                                                    device between units of very different sizes admits them by (AlignGraph_amd); a build that has to grow a capacity takes more */
int agx_unit_upload(agx_unit *u);                /* staged arrays -> HBM: one device block, asynchronous copies behind those of the device's earlier uploads; returns without waiting */
int agx_unit_build(agx_unit *u);                 /* kernels: updateGenomeWithRead/updateKMer (AG:1635-1870, 1353-1624) + filterLowCoverage (AG:1904-1918) */
/* Re-prunes a built unit at another coverage without building it again.  After the call the unit is, in everything a caller can observe, what agx_unit_build leaves on a unit
 * created with `coverage` in agx_params and given the same inputs: the walk graph (agx_unit_walk_graph, both forms), the three outputs of agx_unit_finish byte for byte,
 * agx_stats n_walk_ids / n_special / download_bytes, agx_unit_unitigs, the id map of agx_unit_unitigs_mapped and the stretches of the next finish.  agx_unit_graph and the
 * exports at an explicit threshold (agx_unit_unitigs_region) do not change: they never looked at the prune.  The unit's coverage is the new one from then on: a later
 * agx_unit_build, or agx_unit_upload + build, uses it.  Costs one kernel over the positions and a second run of the walk preparation; agx_stats
 * reprune_attempts and ms_reprune describe the last call.
 * AGX_E_ARG, with the reason in agx_unit_error, unless: the unit is built; it was created with AGX_FLAG_KEEP_COUNTS (the per-node coverage stays on the device only then); it is
 * not trimmed and not released; coverage <= 0x7FFFFFFF (the prune compares signed numbers, as the build does).  A unit that has been downloaded or finished may be re-pruned:
 * it is "not downloaded" again, and the next finish downloads the new walk graph.  AGX_FLAG_ONE_SHOT units only before their download or finish (their landing memory is
 * used once).  The stretches kept by AGX_FLAG_KEEP_PATHS are dropped.  A refused call leaves the unit as it was. */
int agx_unit_reprune(agx_unit *u, uint32_t coverage);
int agx_unit_download(agx_unit *u);              /* HBM -> pinned host memory (the whole walk graph; returns when it is there).  Only needed by a caller that wants the unit's HBM back
                                                    before the walk (agx_unit_trim): agx_unit_finish downloads what has not been downloaded, and does it better */
int agx_unit_finish(agx_unit *u, agx_result *r); /* extdContigs1/2 + scaffoldContigs (AG:1954-2464) on the host.  On a unit that has not been downloaded (r06) the download is STREAMED: the
                                                    walk graph comes down in position windows from the front and the walk begins on what has landed — the walkers of a large unit wait for
                                                    their windows, the first one for all of them (csrc/agx_engine.cpp: begin_streamed_download; AGX_NO_STREAM_DOWNLOAD=1: the whole download first) */
void agx_result_free(agx_result *r);               /* (the buffers are malloc'd; the library keeps up to 16 GB of the ones given back here for the outputs of the next units — fresh memory for them is a
                                                    sixth of a whole-human job's host CPU time —, agx_pool_trim(-1) frees them) */
int agx_unit_trim(agx_unit *u, uint64_t *freed);  /* after agx_unit_download: gives the part of the unit's HBM that the host walk cannot ask for (three quarters of it) back to the device's memory
                                                    region, so that the next unit is admitted when this one's DOWNLOAD is done, not when its walk is; *freed = bytes given back (0: nothing to give —
                                                    small units on a device without a region).  The unit is no longer built afterwards: agx_unit_finish still works, another build uploads again */
int agx_unit_release(agx_unit *u);               /* gives the unit's HBM and download buffers back to the library's caches; the staged inputs stay: upload again = a new unit (not AGX_FLAG_ONE_SHOT units: their inputs are gone after the download) */
void agx_pool_trim(int device);                  /* device >= 0: frees the cached HBM blocks of that device; -1: frees the cached (and retired) pinned host blocks;
                                                    -2: retires the cached pinned host blocks (never handed out again, unmapped by the next -1): what a
                                                    measurement loop uses so that every job maps and registers fresh buffers without paying for unmapping old ones */

int agx_unit_stats(const agx_unit *u, agx_stats *s);
int agx_unit_graph(agx_unit *u, agx_graph *g);   /* after agx_unit_build */
void agx_graph_free(agx_graph *g);
/* Test and inspection hook, like agx_unit_graph: builds the unit if need be, then does a WHOLE download (streamed == 0: the one-piece form of agx_unit_download, which a trimmed unit's
 * walk reads; streamed != 0: the window-by-window form agx_unit_finish uses, waited for to its last piece; AGX_E_ARG where that form does not apply) and copies out what the walk
 * would be handed, before any walk has marked it.  Costs a download and a host copy of every array.  With want_all_node it also fetches the WHOLE record table in two calls of
 * the path the walk fetches single records by (rows of 64 ids, then the rest): that grows the unit's device fetch buffer to n_ids records (32 bytes per id of HBM, kept until
 * agx_unit_release) and moves the end of what agx_unit_trim keeps behind it, so a later trim gives back that much less, or nothing if the buffer fell into a later block.  The unit
 * stays usable: agx_unit_finish afterwards gives what it gives without this call.  Refused (AGX_E_ARG) for AGX_FLAG_ONE_SHOT units: their download lands in the staged
 * inputs and cannot be made twice. */
int agx_unit_walk_graph(agx_unit *u, int streamed, agx_walk_graph *g);
void agx_walk_graph_free(agx_walk_graph *g);
/* Test and inspection hook: copies the front of the last build out of HBM (agx_front above).  After agx_unit_build, before anything that gives the arrays away: AGX_E_ARG
 * on a unit that is not built, after agx_unit_download, agx_unit_trim or agx_unit_release, and for AGX_FLAG_ONE_SHOT units.  The copies are queued on the device's download
 * stream and waited for; nothing is allocated on the device and a build that does not call this pays nothing for it. */
int agx_unit_front(agx_unit *u, agx_front *f);
void agx_front_free(agx_front *f);
/* After agx_unit_build of a unit created with AGX_FLAG_KEEP_COUNTS, before agx_unit_trim / agx_unit_release (AGX_FLAG_ONE_SHOT units: before their download
 * or finish).  Runs on the device over the node table the build left there and changes nothing the walk reads.  AGX_E_ARG otherwise. */
int agx_unit_unitigs(agx_unit *u, agx_unitigs *t);
/* The same export for a window of the unit at a coverage of the caller's choice, at a cost that follows the window.  A node is in it iff its position lies in
 * [pos_lo, pos_hi) and (contigID != -1 or coverage >= min_coverage): the build's pruning rule with min_coverage in place of the build's coverage.  An edge is in it iff
 * both of its ends are (an edge across the window's border is dropped); unitigs, bases, coverage sums, links and their order are DESIGN.md §11's on that sub-graph.
 * head_pos stays the absolute position and head_var the index among ALL of the position's variants, so a segment keeps its GFA name whatever the window and threshold.
 * The node table keeps the edges of the nodes the build pruned, so every min_coverage is served, also one below the build's coverage (0: nothing is pruned).
 * Preconditions and error codes of agx_unit_unitigs; pos_lo > pos_hi or pos_hi > the unit's positions: AGX_E_ARG.  pos_lo == pos_hi gives no segments. */
int agx_unit_unitigs_region(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t);
/* The region export plus the id map of what it exported (agx_idmap above): the join between the walk's ids and the export's segments, made on the device, where the per-node
 * arrays live.  Preconditions of agx_unit_unitigs_region, and the unit was created with AGX_FLAG_KEEP_PATHS as well (AGX_E_ARG otherwise).  t is what
 * agx_unit_unitigs_region gives for the same arguments. */
int agx_unit_unitigs_mapped(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t, agx_idmap *m);
void agx_idmap_free(agx_idmap *m);
/* Edge support of a built unit created with AGX_FLAG_EDGE_SUPPORT.  Preconditions of agx_unit_front (built; not downloaded, trimmed or released; not AGX_FLAG_ONE_SHOT) plus the
 * flag: AGX_E_ARG with the reason otherwise, and a refused call leaves the unit as it was.  The first call after a build zeroes the counters and runs one kernel over the tile
 * lists (agx_k_edge_support); the counters then stay valid until the next build, upload or release (agx_unit_reprune does not touch them), and later calls only convert.
 * A contribution that finds no edge is AGX_E_DEVICE ("internal:").  The conversion to agx_unit_graph's numbering is done on the host and costs what that call's does. */
int agx_unit_edge_support(agx_unit *u, agx_edge_support *s);
void agx_edge_support_free(agx_edge_support *s);
/* agx_unit_unitigs_region (m == NULL) or agx_unit_unitigs_mapped (m != NULL) plus, for every link of t, the support of its edge: from the LAST node of segment link_from[i] to the
 * head node of segment link_to[i].  The number is the edge's own: it does not depend on the window or the threshold.  t and m are what the calls without support give for the
 * same arguments.  Preconditions of agx_unit_edge_support and of the export (AGX_FLAG_KEEP_COUNTS; AGX_FLAG_KEEP_PATHS when m != NULL).  *link_support: [t->n_links], malloc'd,
 * free it with agx_link_support_free (never NULL after AGX_OK, also without links). */
int agx_unit_unitigs_support(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, agx_unitigs *t, uint32_t **link_support, agx_idmap *m);
void agx_link_support_free(uint32_t *link_support);
/* The hits behind the selected edges of a window (agx_edge_reads above).  Preconditions of agx_unit_edge_support (built; not downloaded, trimmed or released; not
 * AGX_FLAG_ONE_SHOT; AGX_FLAG_EDGE_SUPPORT) and AGX_FLAG_KEEP_COUNTS as well (the scratch is the export's, which only such units reserve): AGX_E_ARG with the reason otherwise;
 * pos_lo > pos_hi or pos_hi > the unit's positions: AGX_E_ARG; pos_lo == pos_hi gives an empty table.  A refused call leaves the unit as it was.  The counters are made first
 * if need be (agx_unit_edge_support's first call).  Runs on the device over the tiles of the window only, in chunks of tiles: a count pass, a scan and an emit pass per chunk
 * out of the export's scratch (no allocation; the chunk is halved until its records fit, AGX_EDGE_READS_CHUNK=<tiles> forces a size; a single tile whose records do not fit,
 * and 2^32 listed hits or more, are AGX_E_UNSUPPORTED).  A contribution without an edge, or an emit pass that disagrees with its count, is AGX_E_DEVICE ("internal:").
 * Writes nothing a walk or an export reads. */
int  agx_unit_edge_reads(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t max_support, agx_edge_reads *r);
void agx_edge_reads_free(agx_edge_reads *r);
/* Host only: one line per edge, <unit> <tab> src_pos <tab> src_var <tab> dst_pos <tab> dst_var <tab> support <tab> hit,hit,... (no header line; an edge without hits ends in
 * an empty field); *text is malloc'd, free it with agx_text_free. */
int  agx_edge_reads_tsv(const agx_edge_reads *r, int unit, char **text, size_t *len);
/* The stretches the last agx_unit_finish kept (AGX_FLAG_KEEP_PATHS).  Valid after a finish, also of trimmed and one-shot units, until the next finish, upload, reprune or release;
 * AGX_E_ARG without the flag or before a finish.  The caller gets copies. */
int agx_unit_walk_paths(agx_unit *u, agx_walk_paths *w);
void agx_walk_paths_free(agx_walk_paths *w);
/* The evidence under the records of w (agx_walk_evidence above): normally the table agx_unit_walk_paths returned after the last finish, but any table that passes the checks
 * is served — st_off rises from 0 to n_stretches; id_first <= id_last < the unit's walk ids; every stretch inside its record; a record's stretches in base order without
 * overlap; joined = 1 only directly behind the previous stretch of the same record (AGX_E_ARG with the reason otherwise; AGX_E_UNSUPPORTED for 2^32 graph bases or more, or a
 * record of 2^32 bases or more: offsets are 32-bit).  Preconditions of agx_unit_unitigs_region (AGX_FLAG_KEEP_COUNTS; built and not trimmed; one-shot units before their
 * download); allowed after agx_unit_finish; AGX_FLAG_KEEP_PATHS is not needed.  With AGX_FLAG_EDGE_SUPPORT the counters are made first if need be, under
 * agx_unit_edge_support's preconditions; without it every step is 0xFFFFFFFF, n_steps and n_steps_without_edge are 0 and a non-zero min_support is AGX_E_ARG.  want_tracks
 * != 0 needs rec_lo <= rec_hi <= n_recs.  Runs on the device out of the export's scratch (no allocation; a table too large for it goes through in chunks of bases,
 * AGX_EVIDENCE_CHUNK=<bases> forces a chunk size) and writes nothing the walk or an export reads.  A refused call leaves the unit as it was. */
int agx_unit_walk_evidence(agx_unit *u, const agx_walk_paths *w, uint32_t min_depth, uint32_t min_support,
                           uint32_t want_tracks, uint32_t rec_lo, uint32_t rec_hi, agx_walk_evidence *e);
void agx_walk_evidence_free(agx_walk_evidence *e);
/* Host only: the weak intervals as BED, one line per interval: p<unit>_<rec> <tab> base_first <tab> base_last + 1 <tab> weak <tab> 0 <tab> + <tab> dm:i:<depth_min> <tab>
 * sm:i:<step_min>, "." in place of a number that is 0xFFFFFFFF; *text is malloc'd, free it with agx_text_free. */
int agx_walk_evidence_bed(const agx_walk_evidence *e, int unit, char **text, size_t *len);
/* Pair span: the read pairs across each position.  A KEPT hit is one whose derived record has AGX_HF_SKIP clear (the hits that make events, §13).  Its
 * FRAGMENT runs from f_lo, the smallest, to f_hi, the largest reference position either mate is aligned to (a simple mate: [t0, t0 + len - 1]; a mate with runs: the
 * union of [t, t + n - 1] over its runs), whichever mate lies left; f_hi is clamped to n_pos - 1, and a kept hit with f_lo >= n_pos has no fragment and is counted in
 * n_outside (0 for anything the loaders make).  pairs(x, y), x < y: the fragments with f_lo <= x and y <= f_hi.  span[x - pos_lo]: the fragments with f_lo <= x <= f_hi;
 * cross[x - pos_lo] = pairs(x, x + 1) = span less the fragments that end on x (0 at n_pos - 1).  n_kept and n_outside are the unit's, n_fragments counts the fragments
 * that meet the window.  Nothing depends on the coverage threshold, on a reprune or on the node table.  malloc'd; free with agx_pair_span_free. */
typedef struct { uint32_t pos_lo, pos_hi; uint64_t n_kept, n_fragments, n_outside;
                 uint32_t *span, *cross; } agx_pair_span;                            /* [pos_hi - pos_lo] each */
/* The pair span of positions [pos_lo, pos_hi): pos_lo <= pos_hi <= n_pos (AGX_E_ARG otherwise; pos_lo == pos_hi: an empty table with the unit's n_kept and n_outside).
 * Needs AGX_FLAG_KEEP_COUNTS (the scratch is the export's buffer) and the arrays the edge counting reads: the unit is built, not one-shot, and neither downloaded by
 * agx_unit_download nor trimmed nor released (AGX_E_ARG with the reason); allowed after agx_unit_finish; AGX_FLAG_EDGE_SUPPORT and AGX_FLAG_KEEP_PATHS are not needed.
 * On the device, out of the export's scratch: no allocation, about 12 bytes per position of the window; a window that does not fit goes through in sub-windows (halved
 * until they fit; AGX_SPAN_CHUNK=<positions> forces a size), each one more pass over all hits.  Nothing is kept between calls; nothing a walk or an export reads is
 * written; a refused call leaves the unit as it was. */
int  agx_unit_pair_span(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, agx_pair_span *s);
void agx_pair_span_free(agx_pair_span *s);
/* Pair span under the records of a stretch table w (layout, checks, "graph base" and "step" exactly as agx_walk_evidence above).  The POSITION of walk id a is a for
 * a < n_pos, else the side id's position; an id needs no node to have one, so every graph base has a span.  A step from a base at position x to one at position y has
 * step = pairs(x, y) when y > x — it needs no edge in the node table —, else 0xFFFFFFFF, counted in n_steps_not_forward (0 for the stretches of a finish); n_jump_steps
 * counts the steps with y > x + 1.  A base is THIN iff its span is below min_span or its step is a number below min_span; the thin intervals are maximal runs of thin
 * bases of one record at consecutive base offsets, by (rec, first), with the smallest span and the smallest numbered step inside (min_span = 0: none).  Per record: graph
 * bases, numbered steps, the span summed, the smallest span and the smallest numbered step, each with the smallest base offset that has it (value 0xFFFFFFFF, offset 0:
 * none).  Tracks (want_tracks): pos, span and step per graph base of the records [rec_lo, rec_hi) in stretch order, track_off as in agx_walk_evidence.
 * malloc'd; free with agx_walk_span_free. */
typedef struct { uint32_t n_recs, n_intervals; uint64_t n_graph_bases, n_steps, n_jump_steps, n_steps_not_forward;
                 /* [n_recs] */ uint64_t *rec_graph_bases, *rec_steps, *rec_span_sum; uint32_t *rec_span_min, *rec_span_min_at, *rec_step_min, *rec_step_min_at;
                 /* [n_intervals] */ uint32_t *iv_rec, *iv_first, *iv_last, *iv_span_min, *iv_step_min;
                 /* tracks, want_tracks only */ uint32_t rec_lo, rec_hi; uint64_t n_track; uint64_t *track_off; uint32_t *pos, *span, *step; } agx_walk_span;
/* The pair span under the records of w: the table checks of agx_unit_walk_evidence and the preconditions of agx_unit_pair_span (AGX_E_ARG with the reason).  On the device
 * out of the export's scratch: the whole unit's span and cross (8 bytes per position, made as agx_unit_pair_span makes them, in sub-windows where need be) beside the
 * arrays of one chunk of graph bases (AGX_SPAN_BASE_CHUNK=<bases> forces a chunk size); a unit whose fixed part does not fit is AGX_E_UNSUPPORTED.  The jumps of a chunk
 * go to the host once, are sorted and merged there, and cost one more pass over all hits (skipped for a chunk without jumps): the cost of a table with jumps grows with
 * the number of chunks — a forced chunk of 64 bases means up to one pass over the hits per 64 bases —, and inside the pass a hit walks every entry whose x lies in its fragment.  Nothing is kept between calls; nothing a
 * walk or an export reads is written; a refused call leaves the unit as it was. */
int  agx_unit_walk_span(agx_unit *u, const agx_walk_paths *w, uint32_t min_span, uint32_t want_tracks, uint32_t rec_lo, uint32_t rec_hi, agx_walk_span *e);
void agx_walk_span_free(agx_walk_span *e);
/* Host only: the thin intervals as BED, one line per interval: p<unit>_<rec> <tab> base_first <tab> base_last + 1 <tab> thin <tab> 0 <tab> + <tab> pm:i:<span_min> <tab>
 * jm:i:<step_min>, "." in place of a number that is 0xFFFFFFFF; *text is malloc'd, free it with agx_text_free. */
int  agx_walk_span_bed(const agx_walk_span *e, int unit, char **text, size_t *len);
/* Mate links: the read pairs that join two records of a stretch table w (layout, checks and "graph base" exactly as agx_walk_evidence above; position of
 * a walk id, kept hit, fragment [f_lo, f_hi], n_kept and n_outside as in the pair span).  own[x] is the smallest record with a graph base at position x, or none: n_owned
 * counts the positions with an owner, n_shadowed the graph bases whose record does not own their position.  With A = own[f_lo] and B = own[f_hi] a fragment is UNOWNED (both
 * none), INSIDE (A == B, a record), OPEN TO THE RIGHT (B none; counted on A), OPEN TO THE LEFT (A none; counted on B) or a pair of the LINK (A, B), A the record under the left
 * end: (A, B) and (B, A) are two links.  n_fragments = n_kept - n_outside = n_unowned + n_inside + n_open + n_link_pairs; n_links_all counts the distinct links.  Per record
 * the pairs inside, open to either side, and of the links that leave it (it is A) and reach it (it is B), all before any threshold.  Per link of the table: the pairs, the
 * sum of f_hi - f_lo + 1, and the smallest and largest f_lo and f_hi.  The table holds the links with n_pairs >= min_pairs (0 and 1: all) by (a, b); nothing else depends on
 * min_pairs.  Nothing depends on the coverage threshold, on a reprune or on the node table.  n_passes, n_slots, ms: how the call went (below); agx_stats is as it was.  malloc'd; free with
 * agx_mate_links_free. */
typedef struct { uint64_t n_kept, n_outside, n_fragments, n_unowned, n_inside, n_open, n_link_pairs, n_links_all, n_owned, n_shadowed;
                 uint32_t n_recs, n_links, n_passes, n_slots; double ms;      /* ms: host wall time of the call, from entry to the tables being in the caller's memory */
                 /* [n_recs] */ uint32_t *rec_inside, *rec_open_left, *rec_open_right, *rec_links_out, *rec_links_in;
                 /* [n_links] */ uint32_t *a, *b, *n_pairs; uint64_t *len_sum; uint32_t *lo_min, *lo_max, *hi_min, *hi_max; } agx_mate_links;
/* The mate links of w: the table checks of agx_unit_walk_evidence and the preconditions of agx_unit_pair_span (AGX_E_ARG with the reason).  On the device out of the
 * export's scratch, no allocation: own (4 bytes per position), the per-record counters, and a hash table of the links keyed by (A, B) at 80 bytes per slot with its
 * compacted copy — twice the keys there can be, or the largest power of two that fits; AGX_LINKS_SLOTS=<n> forces a slot count (a power of two from 2; AGX_E_ARG
 * otherwise).  One pass over all hits fills it.  A pass in which a pair finds no slot is discarded and the records it took links from are halved: EVERY PASS IS ONE MORE
 * READ OF ALL HITS (n_passes); a single record whose links do not fit, a unit whose own and table do not fit the scratch, and 2^32 links or more are AGX_E_UNSUPPORTED.
 * Nothing is kept between calls; nothing a walk or an export reads is written; a refused call leaves the unit as it was. */
int  agx_unit_mate_links(agx_unit *u, const agx_walk_paths *w, uint32_t min_pairs, agx_mate_links *l);
void agx_mate_links_free(agx_mate_links *l);
/* Host only: the links as text, one line per link in the table's order and no header line: p<unit>_<a> <tab> p<unit>_<b> <tab> n_pairs <tab> len_sum <tab> lo_min <tab>
 * lo_max <tab> hi_min <tab> hi_max (the names are the BED's and the P lines'); *text is malloc'd, free it with agx_text_free. */
int  agx_mate_links_tsv(const agx_mate_links *l, int unit, char **text, size_t *len);
/* Bubbles: the forks of a region export's graph and what closes them.  The graph is exactly agx_unit_unitigs_region's for the same window and threshold, in its
 * numbering: out(s) are the links that leave segment s in the table's order (by target), in(s) the number of links that enter it.  A FORK is a segment S with k = |out(S)| >= 2.
 * A target X of S with in(X) == 1 is a BRANCH SEGMENT, and its exit is the target of its one link when |out(X)| == 1; a target with in(X) >= 2 is a DIRECT branch (no segment)
 * with exit X itself.  The class of a fork is the first that applies of: TIP (a branch segment has no link), NESTED (a branch segment has two links or more), SINKS_DIFFER (the
 * exits are not all one segment), SINK_SHARED (the common exit T has in(T) > k), BUBBLE with sink T.  n_forks = n_bubbles_all + n_tip + n_nested + n_sinks_differ + n_sink_shared;
 * longest_branch: the most nodes of a branch segment of any bubble.  None of these depends on max_nodes.  The table holds the bubbles whose every branch segment has at most
 * max_nodes nodes (0xFFFFFFFF: all), ordered by source segment; bubble i has the branch rows br_off[i] .. br_off[i + 1), in out(S)'s order.  A direct branch's row has br_pos =
 * br_var = 0xFFFFFFFF, no nodes, coverage or bases; br_sup_in is the support of the link S -> X, br_sup_out of the link X -> T (a direct branch: the same link), both NULL without
 * support.  Positions and variants are the whole unit's (the S lines' names), so nothing depends on the window or threshold except through the sub-graph: a fork cut by the
 * window's border is a TIP, or no fork.  ms, bytes_down: how the call went (agx_unit_bubbles; 0 from the host-only twin).  malloc'd; free with agx_bubbles_free. */
typedef struct { uint32_t n_segs, n_links;                       /* the sub-graph's */
                 uint64_t n_forks, n_bubbles_all, n_tip, n_nested, n_sinks_differ, n_sink_shared;
                 uint32_t longest_branch, max_nodes, has_support, n_bubbles, n_branches; uint64_t n_bases, bytes_down; double ms;
                 /* [n_bubbles] */ uint32_t *src_pos, *src_var, *src_last, *sink_pos, *sink_var; /* [n_bubbles + 1] */ uint32_t *br_off;
                 /* [n_branches] */ uint32_t *br_pos, *br_var, *br_nodes; uint64_t *br_cov; /* [n_branches + 1] */ uint64_t *br_seq_off; uint32_t *br_sup_in, *br_sup_out;
                 char *seq; } agx_bubbles;                        /* [n_bases] the branch segments' bases, row after row */
/* The bubbles of the window [pos_lo, pos_hi) at min_coverage, found on the device: the region export's front up to its phase 3, then a pass over the links and one over the
 * segments where they lie, three scans, and the rows — the segment table is never downloaded.  Preconditions and refusals of agx_unit_unitigs_region; want_support != 0:
 * also those of agx_unit_edge_support (AGX_FLAG_EDGE_SUPPORT; the counters are made first if need be).  Three more arrays per segment and the rows are carved from what the
 * export no longer reads behind phase 3: no allocation (with support: the per-link array agx_unit_unitigs_support keeps); a graph whose rows do not fit there is
 * AGX_E_UNSUPPORTED.  Totals that break the identity above, or a table index out of range, are AGX_E_DEVICE ("internal:").  agx_stats is as it was (the wall time is the
 * answer's ms); nothing a walk or an export reads is written; a refused call leaves the unit as it was. */
int  agx_unit_bubbles(agx_unit *u, uint32_t pos_lo, uint32_t pos_hi, uint32_t min_coverage, uint32_t max_nodes, uint32_t want_support, agx_bubbles *b);
/* Host only, the same table from an export the caller holds (and the CPU replay of the call above: both class a fork with one function, agx_bubble_class).  link_support: the
 * array agx_unit_unitigs_support gave with t, or NULL.  AGX_E_ARG for a table that does not describe itself: links not ordered by source, a segment past n_segs, offsets that fall. */
int  agx_unitigs_bubbles(const agx_unitigs *t, const uint32_t *link_support /* may be NULL */, uint32_t max_nodes, agx_bubbles *b);
void agx_bubbles_free(agx_bubbles *b);
/* Host only: one line per bubble in the table's order and no header line, tab-separated: source name, sink name (u<unit>_<pos>_<var>, the S lines'), the source's last
 * position, the sink's head position, k, then six comma lists with an entry per branch: name (* for a direct branch), nodes, coverage, support_in, support_out (. without
 * support), bases (* for a direct branch); *text is malloc'd, free it with agx_text_free. */
int  agx_bubbles_tsv(const agx_bubbles *b, int unit, char **text, size_t *len);
void agx_unitigs_free(agx_unitigs *t);
/* Host only: the S and L lines of GFA 1.0 for unit `unit` (no header line), as DESIGN.md §11 defines them; *text is malloc'd, free it with agx_text_free. */
int agx_unitigs_gfa(const agx_unitigs *t, int unit, char **text, size_t *len);
/* Host only: the bytes of agx_unitigs_gfa with "\tRC:i:<link_support[i]>" appended to the L line of link i (GFA 1.0's read-count tag).  AGX_E_ARG also for link_support == NULL. */
int agx_unitigs_gfa_support(const agx_unitigs *t, const uint32_t *link_support, int unit, char **text, size_t *len);
/* Host only: the P lines of GFA 1.0 that lay the records of w over the segments of t (m: the id map of the same export), as DESIGN.md §11 "Paths" defines them:
 *   P\tp<unit>_<record>_<base_off>\t<seg>+,<seg>+,...\t*\tln:i:<nodes>\tfs:i:<rank of the first node in the first segment>\tls:i:<rank of the last node in the last segment>
 * one line per maximal piece of a record's node sequence that stays on edges and inside the map, ordered by (record, first base).  AGX_E_ARG where the three tables do not
 * agree: a consecutive pair of nodes must be (same segment, rank + 1) or (a segment's last node -> rank 0 of the next, with that link in t). */
int agx_unitigs_paths_gfa(const agx_unitigs *t, const agx_idmap *m, const agx_walk_paths *w, int unit, char **text, size_t *len);
void agx_text_free(char *text);

/* The five-call seam in one call.  write_files != 0 also writes the three files under tmp_dir like the reference does. */
int agx_run_unit(const agx_params *p, const char *tmp_dir, int unit, int write_files, agx_result *r, char *err, size_t err_len);
int agx_run_unit_shared(const agx_params *p, const char *tmp_dir, int unit, int write_files, const agx_reads *reads, agx_result *r, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif
#endif /* AGX_H */
