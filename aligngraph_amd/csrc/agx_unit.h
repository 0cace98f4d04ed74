// agx_unit.h — what agx_engine.cpp (a unit's way from its arrays to its output: stage, upload, build, download, finish) and agx_export.cpp (the calls that answer a
// question about a built unit out of the export's scratch) both need: the unit object with the types it is made of, the small helpers both files call, and the
// declarations of the export layouts that size the scratch a unit reserves with its block.  Internal: nothing outside those two files includes it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <mutex>
#include <system_error>
#include <thread>
#include <type_traits>
#include <pthread.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <vector>

#include "agx_host.h"
#include "agx_forms.h"
#include "agx_mem.h"

#include "agx_kargs.h"

using namespace agx;

namespace agx {

#define HIP_OK(expr) AGX_HIP_OK(expr)

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// AGX_TRACE=1: one stderr line per stage of every unit with host times (ms since the first line): who waited for whom in a pipelined job
inline const bool g_trace = getenv("AGX_TRACE") != nullptr;
inline void trace(const void *unit, const char *what, double from_ms, size_t n_pos) {
    if (!g_trace) return;
    static const double t00 = now_ms();
    // (+ the CPU time of the calling thread since its previous line: a stage that waits should cost none)
    static thread_local double cpu_last = 0;
    timespec ts{}; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); const double cpu = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    fprintf(stderr, "[agx trace] unit %p (%zu pos) %-22s %9.2f -> %9.2f ms   (thread cpu +%.2f ms)\n", unit, n_pos, what, from_ms - t00, now_ms() - t00, cpu - cpu_last);
    cpu_last = cpu;
}

// Wait for an event asleep.  hipEventSynchronize spins whatever the event's flags say (ROCm 7.2: the five unit threads of a cfg3 job burned 25 ms of CPU each waiting
// for uploads and builds — a third of the job's CPU time, beside the walkers of the units in front of them, on a box whose control group grants 16 CPUs): a short
// spin for what is about to finish, then queries between short sleeps (a sleep of 20 us takes 70-80 with the default timer slack: that is the price of a wake-up).
inline hipError_t wait_event(hipEvent_t e) {
    static const bool spin = getenv("AGX_SPIN_WAIT") != nullptr;
    if (spin) return hipEventSynchronize(e);
    for (int i = 0; i < 64; i++) { const hipError_t r = hipEventQuery(e); if (r != hipErrorNotReady) return r; }
    for (;;) {
        const timespec ts{0, 20000}; nanosleep(&ts, nullptr);
        const hipError_t r = hipEventQuery(e); if (r != hipErrorNotReady) return r;
    }
}

// Section boundaries of a build on the build streams: the end of one section is the start of the next (one record instead of two: an
// event record costs the stream about as much as a small kernel).
enum { B_START = 0, B_PREP, B_BIN, B_NODE, B_BIG, B_EDGE, B_SLOW, B_COMPACT, B_N };
// (two more events bracket the whole build: Boundaries::first / last)
struct Boundaries {
    hipEvent_t e[B_N] = {}, first = nullptr, last = nullptr; bool at[B_N] = {}; bool all = false;      // at[b]: boundary b was marked in the last build; all: mark every boundary (AGX_FLAG_TIME_SECTIONS)
    void init() { for (auto &x : e) HIP_OK(hipEventCreate(&x)); HIP_OK(hipEventCreate(&first)); HIP_OK(hipEventCreate(&last)); }
    double span() const { float f = 0; return hipEventElapsedTime(&f, first, last) == hipSuccess ? f : 0; }
    void destroy() { for (auto &x : e) { if (x) (void)hipEventDestroy(x); x = nullptr; } if (first) (void)hipEventDestroy(first); if (last) (void)hipEventDestroy(last); first = last = nullptr; }
    void begin() { for (bool &x : at) x = false; }
    void mark(int b, hipStream_t st) { if (!all && b != B_BIN && b != B_NODE) return; HIP_OK(hipEventRecord(e[b], st)); at[b] = true; }      // the node sweep is always timed
    double ms(int b) const { if (!at[b - 1] || !at[b]) return 0; float f = 0; (void)hipEventElapsedTime(&f, e[b - 1], e[b]); return f; }      // section that ends at boundary b
};

// One helper thread per unit, started with the unit and asleep until it is handed work: what a unit can prepare while its upload and
// build run (the pinned download buffers, the output buffers) without its worker waiting for it.  Not started on demand: creating a
// thread maps a stack, and that waits for the address-space lock that another unit's hipHostRegister holds for milliseconds.
struct UnitHelper {
    enum { DL = 0, OUT = 1, WALK = 2, SLOTS = 3 };      // (taken in this order)
    std::thread th; std::mutex m; std::condition_variable cv;
    std::function<void()> job[SLOTS]; bool queued[SLOTS] = {false, false, false}, running[SLOTS] = {false, false, false}; bool stop = false, started = false;
    void start() {
        if (started) return;
        th = std::thread([this] {
            pthread_setname_np(pthread_self(), "agx-helper");
            std::unique_lock<std::mutex> l(m);
            for (;;) {
                cv.wait(l, [this] { return stop || queued[DL] || queued[OUT] || queued[WALK]; });
                if (stop) return;
                const int s = queued[DL] ? DL : queued[OUT] ? OUT : WALK;
                std::function<void()> f = std::move(job[s]); queued[s] = false; running[s] = true;
                l.unlock();
                try { f(); } catch (...) { }
                l.lock(); running[s] = false; cv.notify_all();
            }
        });
        started = true;
    }
    bool submit(int s, std::function<void()> f) {       // false: no helper (the caller does the work itself, later)
        if (!started) return false;
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !queued[s] && !running[s]; });
        job[s] = std::move(f); queued[s] = true; cv.notify_all();
        return true;
    }
    void wait(int s) { if (!started) return; std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !queued[s] && !running[s]; }); }
    ~UnitHelper() { if (started) { { std::lock_guard<std::mutex> l(m); stop = true; } cv.notify_all(); th.join(); } }
};

// Which forms a unit's read alignments and its sequence cross PCIe in (agx_forms.h; DESIGN.md "Upload forms"), read from the environment ONCE per entry — where a unit's
// files are loaded and where its inputs are staged — and kept in the unit: the loaders' buffers, the packers and the steps of finish_staging all see the same answer.
//   tiled     tile-ordered records and rows (AGX_NO_TILED_UPLOAD, set at all: the file-order forms)
//   row_diff  the read rows as differences from the reference (AGX_ROW_DIFF=1; it is NOT the default: agx_engine.cpp, stage_rows)
//   compact   hit and side records in their compact wire forms (AGX_WIRE_PLAIN=1: the records as they are; A/B, tests)
//   ref_raw   the unit sequence as its bytes (AGX_REF_RAW, set at all)
//   windows   upload windows of the first build's sweep (AGX_UPLOAD_WINDOWS: tests); 0: by size
struct UploadChoice { bool tiled = true, row_diff = false, compact = true, ref_raw = false; unsigned windows = 0; };
inline UploadChoice upload_choice() {
    UploadChoice c;
    const char *diff = getenv("AGX_ROW_DIFF"), *plain = getenv("AGX_WIRE_PLAIN"), *win = getenv("AGX_UPLOAD_WINDOWS");
    c.tiled = !getenv("AGX_NO_TILED_UPLOAD"); c.ref_raw = getenv("AGX_REF_RAW") != nullptr;
    c.row_diff = diff && atoi(diff) != 0; c.compact = !(plain && atoi(plain) != 0);
    c.windows = win ? std::max(1u, (unsigned)atoi(win)) : 0u;      // (a forced 0 was always one window)
    return c;
}

// units of this process that are uploaded and not yet walked: the walk of the LAST one runs alone (the tail of a job) and may take every walker there is
inline std::atomic<int> g_walks_pending{0};

}  // namespace agx

struct agx_unit {
    agx_params prm{};
    std::string err;
    UploadChoice choice;                // the upload forms this unit takes (read where its files are loaded and where its inputs are staged)
    Threads T; Pairs P;                 // what the loaders / the packed-array calls filled (empty when the unit came out of a cache file)
    UnitView V;                         // what everything downstream reads: into T / P, or into the mapped cache file
    size_t n_chain_str = 0;             // bytes behind V.chain_str (agx_unit_walk_graph hands them out)
    struct Mapped { void *p = nullptr; size_t n = 0; void reset() { if (p) munmap(p, n); p = nullptr; n = 0; } ~Mapped() { reset(); } } cache_map;
    agx_u32 n_seg0 = 0, stride = 0, n_slots = 0, n_rows = 0; unsigned long long pairs_in_file = 0, sam_pairs = 0;
    bool have_ref = false, have_threads = false, staged = false, uploaded = false, built = false, downloaded = false;
    bool consumed = false;             // AGX_FLAG_ONE_SHOT: the download has overwritten the staged inputs
    bool pending_walk = false;         // counted in g_walks_pending: uploaded, not yet walked (or released)
    bool trimmed = false;              // agx_unit_trim since the last build: the node table may be gone (agx_unit_unitigs refuses)
    bool expanded = false;             // the conti-mer tables and vote codes have been made from what was uploaded (opens the unit's first build)
    hipEvent_t ev_built = nullptr;     // this unit's build commands are done (waited for on the host; ev_dl: its download)
    UnitOutput out; OutBuf out_initial; bool out_ready = false;      // output buffers of the next finish, reserved and touched by a helper thread while the unit is uploaded and built (prepare_outputs)
    UnitHelper helper;
    hsa_signal_t dl_signal{}; hsa_agent_t dl_agent{}; bool dl_sdma = false;      // downloads by the SDMA engines (HsaCopy)
    // streamed download (begin_streamed_download): piece 0 = what the walk needs before it can plan (side positions, overflow edges), 1 .. n = position windows from the front,
    // n + 1 = the bases; cut_main / cut_side: the ids in front of window w (entry n: all of them)
    enum { DL_SIGNALS = AGX_DL_PIECES + 2 };
    hsa_signal_t dl_piece[DL_SIGNALS] = {}; bool dl_piece_made = false, dl_streaming = false; agx_cut_args cuts{}; agx_u32 cut_main[AGX_DL_PIECES + 1] = {}, cut_side[AGX_DL_PIECES + 1] = {};
    double dl_t0 = 0, dl_est_ms = 0; size_t dl_stream_bytes = 0; std::atomic<bool> dl_timed{false};
    DevArena arena;
    // staged inputs: what the device wants of T and P, in pinned memory (stage_inputs)
    PBuf<agx_whit> s_hits; PBuf<agx_wside> s_sides; PBuf<agx_wrun> s_runs; PBuf<agx_u8> s_codes; PBuf<unsigned long long> s_other; PBuf<agx_u32> s_jump; size_t n_other = 0, n_sides = 0, n_jump = 0;      // the read alignments in the wire formats of agx_core.h
    PBuf<agx_u8> s_ref; PBuf<agx_refx> s_refx; size_t n_refx = 0; bool ref_packed = false;      // the unit sequence: 2 bits per base + the stretches of other bytes (ref_packed), or the bytes as they are
    PBuf<agx_u32> s_chain_end, s_region_off; PBuf<agx_cmseg> s_segs; size_t n_segs = 0;
    // r06, tile-ordered upload (stage_tiled; agx_forms.h: gather_tiled): the wire records and the read rows in the order of the hits' first tiles — what the device is sent instead of s_hits / s_perm / s_codes / s_other
    PBuf<agx_whit> s_hits_t; PBuf<agx_u8> s_codes_t; PBuf<unsigned long long> s_other_t; size_t n_other_t = 0; bool tiled = false; std::vector<agx_u32> slot_row;      // slot_row[i] = staged row of the i-th hit's left mate (the walk's k-mer tails)
    // the hit and side records in their compact wire forms (agx_core.h; made at the end of staging: stage_tiled or stage_wire_hits, stage_wire_sides; agx_forms.h).  hits_compact / sides_compact = false:
    // the unit sends the 16- and 12-byte records themselves (nothing gained, a run pool that is not in side order, AGX_WIRE_PLAIN=1)
    // s_wire: the hits' blocks, escapes and extra words in one pinned buffer of the records' size (or, tile-ordered with nothing gained, the records); s_csides: counts, then the listed sides
    PBuf<char> s_wire, s_csides; const agx_whit *wire_esc = nullptr; const agx_u32 *wire_ext = nullptr; const agx_cside_esc *wire_listed = nullptr; size_t n_cblocks = 0, n_cesc = 0, n_cext = 0, n_csesc = 0; agx_u32 side_first = 0; bool hits_compact = false, sides_compact = false;
    agx_u32 front_windows = 1;      // windows the last build's node sweep ran in (agx_unit_front)
    agx_u32 n_win = 1, win_tile[9] = {};      // a unit's first build sweeps windows of tiles as their rows land: window w = tiles [win_tile[w], win_tile[w + 1])
    hipEvent_t ev_rows[8] = {}, ev_win[8] = {}, ev_sw0[8] = {}, ev_sw1[8] = {};      // rows of window w in HBM / expanded; around window w's sweep (its time is the sum over the windows)
    PBuf<agx_u32> s_perm, s_tfirst, s_jump_at; agx_u32 lookback = 2;      // the hits in the order of their first tile (stage_order): perm[i] = the i-th hit of that order, tile_first[t] = hits in front of tile t's own; pass J's hits as places in it
    PBuf<char> s_landing;               // one-shot units: what the download needs beyond the dead staged inputs it lands in, pinned when the unit is staged (not inside T_core)
    PBuf<agx_cntrun> s_cntruns; PBuf<agx_chunk> s_cntchunks, s_segchunks; PBuf<agx_u32> s_segindex; size_t n_cntruns = 0, n_cntchunks = 0, n_segchunks = 0, n_segindex = 0;      // what the device builds the conti-mer tables from (build_cm_layout)
    // the read rows in their upload form (agx_core.h "read rows relative to the reference"; made at the end of staging: stage_rows): count byte per row, offsets of the
    // 64-row blocks in the stream, the stream of 16-bit units, one bit per hit (its row's anchor).  rows_diffed = false: the rows cross as their 2-bit classes (s_codes)
    PBuf<agx_u16> s_units; PBuf<agx_u8> s_rowcnt; PBuf<agx_u32> s_blockoff, s_blockfirst, s_anchor; size_t n_units = 0, n_rowcnt = 0, n_blockoff = 0, n_blockfirst = 0, n_anchor = 0, n_rows_explicit = 0; bool rows_diffed = false;
    size_t nh = 0, n_runs = 0, n_cm = 0, n_codes = 0; agx_u32 maxlen = 0;      // n_codes: bytes of packed classes (four bases each); n_other: listed bases that are not A, C, G, T
    std::vector<agx_u32> row_slot;      // staged read bases: one row per (pair, a mate) that some hit uses; row -> read slot (general loader / agx_unit_push_pairs)
    std::vector<uint64_t> row_off;      // fast loader: row -> where the read's bases start in the mapped reads file (the bases are never copied: the walk reads the k-mer tails of written records there)
    std::shared_ptr<agx::ReadsIndex> reads_keep;      // the reads file that row_off points into (shared with the caller's agx_reads, or the unit's own)
    std::unique_ptr<agx::FileView> reads_map;          // the same for a unit that came out of its cache file: only the mapping, no index
    bool pairs_staged = false;          // the fast loader has written hits, runs, codes and the list of other bases straight into the staged buffers
    agx::PairsFile pairs_file;          // the unit's read alignments were handed over staged (tmp/_agx_pairs.<u>.bin, agx_host.h): the mapped file, which the walk takes its k-mer tails from
    // inputs on the device
    DBuf<agx_u32> d_cm_start; DBuf<agx_cmkey> d_cm; DBuf<agx_cmhead> d_cm_head; DBuf<char> d_ref; DBuf<agx_cmseg> d_segs;
    DBuf<agx_run> d_runs; DBuf<agx_u8> d_codes, d_vcodes; DBuf<unsigned long long> d_other;
    DBuf<agx_u16> d_units; DBuf<agx_u8> d_rowcnt; DBuf<agx_u32> d_blockoff, d_blockfirst, d_anchor;
    DBuf<agx_cntrun> d_cntruns; DBuf<agx_chunk> d_cntchunks, d_segchunks; DBuf<agx_u32> d_jump, d_segindex;
    DBuf<agx_chit_block> d_chits; DBuf<agx_whit> d_cesc; DBuf<agx_u32> d_cext, d_cside_scan; DBuf<agx_u16> d_csides; DBuf<agx_cside_esc> d_csesc;      // the compact forms of the next line's first two, until the first build has expanded them
    DBuf<agx_whit> d_whits; DBuf<agx_wside> d_wsides; DBuf<agx_wrun> d_wruns; DBuf<agx_u8> d_wref; DBuf<agx_refx> d_refx;      // what was uploaded, until the first build has expanded it
    // derived
    DBuf<agx_dhit> d_dhit; DBuf<agx_u32> d_tile_cnt, d_tile_off, d_cursor, d_unsorted, d_tile_recs, d_scan_tmp, d_words; DBuf<unsigned long long> d_scan_desc; size_t scan_desc_n = 0;      // descriptors of the three one-launch scans   // d_words: counters/status
    // node table
    agx_u32 pool_cap = 0, spill_lo = 0, ovf_cap = 0, list_cap = 0, sp_cap = 0;
    DBuf<agx_u32> d_pool_cnt, d_region_off; agx_u32 n_regions = 0;      // the node pool's slices (AGX_REGION_TILES tiles each) and their counters
    DBuf<agx_u32> d_node_start, d_slow_list, d_perm, d_tfirst, d_ckey, d_long; DBuf<agx_u16> d_node_cnt; DBuf<agx_u8> d_pos_succ;
    DBuf<agx_u32> d_cid, d_coff, d_cid0, d_coff0, d_off0, d_next; DBuf<agx_u8> d_base, d_flags; DBuf<agx_sref> d_sref; DBuf<int> d_counts;
    DBuf<agx_u32> d_e_cnt, d_ovf_cnt, d_sup_tot, d_lsup;      // AGX_FLAG_EDGE_SUPPORT: counters parallel to d_next / d_ovf, per-tile totals (events, contributions, then the unmatched word); d_lsup: the links' numbers of the last export with support (taken when first needed)
    bool support_valid = false; uint64_t sup_events = 0, sup_adds = 0;      // the counters hold the last build's counts (ensure_support)
    DBuf<char> d_ut;                   // the unitig export's scratch (unitig_layout): reserved with the unit's block when it keeps counts, reused by every export
    DBuf<agx_edge_ovf> d_ovf; DBuf<agx_u32> d_mid_list, d_big_list, d_scratch, d_huge_list, d_scratch_huge; bool huge = false, dense = false;      // dense: the scatter fallback of the tile lists is queued (a build met more than AGX_LONG_MAX long hits); huge: pass 3 of the node sweep is queued (a build met a position beyond AGX_MAXV_BIG variants)
    // walk graph (agx_core.h "walk preparation")
    agx_u32 n_ids = 0;
    DBuf<agx_u32> d_side_pk, d_tile_side, d_tile_side_start, d_aid_of; DBuf<char> d_a_str;
    DBuf<agx_u8> d_a_meta, d_a_mark; DBuf<agx_walknode> d_fetch, d_sp_node; DBuf<agx_u32> d_a_nid; DBuf<agx_edge_ovf> d_a_ovf; agx_compact_args walk_args{};      // walk_args: the last build's, for record fetches
    DBuf<agx_u32> d_chain_end, d_side_xpos, d_sp_cnt, d_sp_rank; DBuf<unsigned long long> d_sp_bits;
    agx_u32 n_chain_end = 0, n_special = 0, n_words = 0;
    size_t keep_end = 0;               // where the arrays that outlive the download end in the arena's first block (pool_bufs, fetch_records; do_trim gives back what lies behind)
    // downloaded: the walk graph with its sparse record table (agx_core.h); the full record table stays on the device
    PBuf<char> h_a_str; PBuf<agx_u8> h_a_meta; PBuf<agx_u32> h_side_xpos, h_sp_rank; PBuf<unsigned long long> h_sp_bits;
    PBuf<agx_walknode> h_sp_node, h_fetch; PBuf<agx_edge_ovf> h_a_ovf; PBuf<agx_hop> h_sp_hop; DBuf<agx_hop> d_sp_hop;
    PBuf<agx_u32> h_words;
    agx_u32 n_nodes = 0, n_ovf = 0, n_tiles = 0, n_tile_entries = 0, n_big = 0, n_mid = 0, n_slow = 0;
    Boundaries ev; hipEvent_t ev_front = nullptr, ev_passA = nullptr, ev_passJ = nullptr, ev_up0 = nullptr, ev_uploaded = nullptr, ev_dl = nullptr, ev_hits = nullptr;      // ev_hits: everything but the read bases is in HBM
    bool up_timed = false;
    agx_stats stats{};
    ~agx_unit() {
        arena.reset();                  // (while the views it empties are still there)
        if (pending_walk) g_walks_pending.fetch_sub(1);
        ev.destroy();
        for (hipEvent_t e : {ev_front, ev_passA, ev_passJ, ev_up0, ev_uploaded, ev_dl, ev_built, ev_hits}) if (e) (void)hipEventDestroy(e);
        for (auto *arr : {ev_rows, ev_win, ev_sw0, ev_sw1}) for (int i = 0; i < 8; i++) if (arr[i]) (void)hipEventDestroy(arr[i]);
        if (dl_signal.handle) (void)hsa_signal_destroy(dl_signal);
        if (dl_piece_made) for (hsa_signal_t g : dl_piece) if (g.handle) (void)hsa_signal_destroy(g);
    }
};

namespace agx {

enum { W_CUT = 34 /* [2 * (AGX_DL_PIECES + 1)] the cuts of a streamed download: agx_cut_args */, W_TOTAL = W_CUT + 2 * (AGX_DL_PIECES + 1) };
enum { W_ERR = 0, W_POOL = 1, W_BIGCOUNT = 2, W_STATUS = 3, W_OVFCOUNT = 4, W_SLOWCOUNT = 5, W_LONGCOUNT = 6 /* hits that span more tiles than a list's window looks back over */, W_UNUSED7 = 7, W_MIDCOUNT = 8, W_JUMPCOUNT = 9, W_SPILL = 10, W_HUGECOUNT = 11, W_N = 12 };

inline void fill_sweep_args(agx_unit *u, agx_sweep_args &S) {
    memset(&S, 0, sizeof S);
    S.cm_start = u->d_cm_start.p; S.cm = u->d_cm.p; S.cm_head = u->d_cm_head.p; S.ref = u->d_ref.p;
    S.dhit = u->d_dhit.p; S.runs = u->d_runs.p; S.vcodes = u->d_vcodes.p; S.stride = u->stride;
    S.tile_off = u->d_tile_off.p; S.tile_recs = (decltype(S.tile_recs))u->d_tile_recs.p;
    S.n_pos = (agx_u32)u->V.n_pos; S.n_tiles = u->n_tiles; S.k = u->prm.k; S.iv = (int)u->prm.insert_variation; S.coverage = (int)u->prm.coverage;
    S.node_start = u->d_node_start.p; S.node_cnt = u->d_node_cnt.p; S.pos_succ = u->d_pos_succ.p; S.side_pk = u->d_side_pk.p; S.tile_side = u->d_tile_side.p;
    S.nk_cid = u->d_cid.p; S.nk_coff = u->d_coff.p; S.nk_cid0 = u->d_cid0.p; S.nk_coff0 = u->d_coff0.p; S.nk_off0 = u->d_off0.p;
    S.n_base = u->d_base.p; S.n_flags = u->d_flags.p; S.n_sref = u->d_sref.p; S.n_next = u->d_next.p;
    S.n_counts = (u->prm.flags & AGX_FLAG_KEEP_COUNTS) ? u->d_counts.p : nullptr;
    S.pool_cap = u->pool_cap;
    S.sweep_stats = nullptr;
}
// what the three passes of a build's node sweep take (the window of tiles of pass 0 is the caller's: tile_lo / tile_hi), and its three edge passes
inline void fill_node_args(agx_unit *u, agx_node_kargs &K) {
    agx_u32 *w = u->d_words.p;
    fill_sweep_args(u, K.S);
#ifdef AGX_SWEEP_STATS
    K.S.sweep_stats = w + W_N + 6;
#endif
    K.pool_cnt = u->d_pool_cnt.p; K.region_off = u->d_region_off.p; K.spill_lo = u->spill_lo; K.spill_cnt = w + W_SPILL;
    K.mid_count = w + W_MIDCOUNT; K.mid_list = u->d_mid_list.p; K.mid_n = w + W_MIDCOUNT;
    K.big_count = w + W_BIGCOUNT; K.big_list = u->d_big_list.p; K.status = w + W_STATUS;
    K.list_cap = u->list_cap; K.big_n = w + W_BIGCOUNT; K.scratch = u->d_scratch.p;
    K.slow_list = u->d_slow_list.p; K.slow_count = w + W_SLOWCOUNT; K.fallback_queued = 1u;
    K.huge_count = w + W_HUGECOUNT; K.huge_n = w + W_HUGECOUNT; K.huge_list = u->d_huge_list.p; K.scratch_huge = u->d_scratch_huge.p; K.huge_queued = u->huge ? 1u : 0u;
}
inline void fill_edge_args(agx_unit *u, agx_edge_kargs &E) {
    agx_u32 *w = u->d_words.p;
    fill_sweep_args(u, E.S); E.ovf = u->d_ovf.p; E.ovf_count = w + W_OVFCOUNT; E.ovf_cap = u->ovf_cap; E.list_cap = u->list_cap;
    E.n_hits = (agx_u32)u->nh; E.jump_list = u->d_jump.p; E.n_jump = (agx_u32)u->n_jump; E.abort = w + W_STATUS; E.big_list = u->d_big_list.p; E.big_n = w + W_BIGCOUNT; E.slow_list = u->d_slow_list.p; E.slow_count = w + W_SLOWCOUNT;
}

template <class F> int guarded(agx_unit *u, F f) {
    try { f(); return AGX_OK; }
    catch (const Error &e) { if (u) u->err = e.msg; return e.code ? e.code : AGX_E_ARG; }
    catch (const std::bad_alloc &) { if (u) u->err = "out of host memory"; return AGX_E_ARG; }
    catch (const std::exception &e) { if (u) u->err = e.what(); return AGX_E_ARG; }
}

inline bool keeps_paths(const agx_unit *u) { return (u->prm.flags & (AGX_FLAG_KEEP_PATHS | AGX_FLAG_KEEP_COUNTS)) == (AGX_FLAG_KEEP_PATHS | AGX_FLAG_KEEP_COUNTS); }

// The export layouts that plan_capacities sizes a unit's block by, and the numbering of agx_unit_graph that agx_unit_edge_support shares (agx_export.cpp, agx_engine.cpp)
size_t unitig_layout(size_t cap, size_t n_pos, size_t n_ovf, char *base, agx_unitig_args *A, agx_u32 **words);
size_t unitig_region_layout(size_t cap, size_t n_win, size_t kept, size_t n_ovf, char *base, agx_unitig_region_args *A, agx_u32 **words);
size_t idmap_layout(size_t ids, size_t runs, char *base, agx_idmap_args *A);
size_t mapped_scratch(size_t cap, size_t n_pos, size_t n_nodes, size_t n_ids, size_t n_ovf, size_t *map_at);
void number_nodes(const std::vector<agx_u32> &node_start, const std::vector<agx_u16> &node_cnt, agx_u32 cap, agx_u32 nn, std::vector<agx_u32> &canon, std::vector<agx_u32> &slot_of, uint32_t *start_out);

}  // namespace agx
