// agx_host.h — host-side containers shared by the loader, the engine and the walk.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <string>
#include <system_error>
#include <thread>
#include <vector>
#include "agx_core.h"

namespace agx {

struct Error { int code; std::string msg; };   // thrown inside the library, converted to a return code at the C-ABI

// fn(t) on `threads` threads.  Nothing may leave a worker thread as an exception (it would terminate the process behind a C ABI that promises
// return codes): whatever a worker throws is carried to the caller and rethrown there; a thread that cannot be started just leaves its
// share to be done here.
template <class F> void on_threads(unsigned threads, F fn) {
    std::vector<std::thread> th; std::vector<std::exception_ptr> ex(threads);
    auto guarded = [&](unsigned t) { try { fn(t); } catch (...) { ex[t] = std::current_exception(); } };
    std::vector<unsigned> mine{0u};
    for (unsigned t = 1; t < threads; t++) { try { th.emplace_back(guarded, t); } catch (const std::system_error &) { mine.push_back(t); } }
    for (unsigned t : mine) guarded(t);
    for (auto &x : th) x.join();
    for (auto &e : ex) if (e) std::rethrow_exception(e);
}

// error codes (include/agx.h mirrors these)
enum {
    E_OK = 0, E_IO = -1, E_FORMAT = -2, E_UNSUPPORTED = -3, E_ALIGNMENT = -4, E_DEVICE = -5, E_ARG = -6, E_OVERFLOW = -7, E_NOGPU = -8
};

// full conti-mer (ContiMer, AG:51-62): key for node build + what the walk follows
struct ContiMer { char nuc; agx_u32 cid, coff, next_off, next_item; };   // next_off == NONE: chain end

// Result of contig threading (updateGenomeWithContig, AG:884-1217) for one unit
struct Threads {
    std::string ref;                       // reference bases followed by the positions appended for contig insertions (AG:1016, 1036)
    agx_u32 n_ref = 0;                     // length of the original unit sequence
    std::vector<agx_u32> cm_start;         // [n_pos+1]   (general loader only; the fast loader keeps counts and runs)
    std::vector<ContiMer> cm;              //             (general loader only)
    std::vector<agx_u8> cm_cnt;            // [n_pos] conti-mers per position
    size_t n_cm = 0;                       // conti-mers in all (= cm.size() where cm is kept)
    std::string initial_contigs;           // bytes of tmp/_initial_contigs.<u>.fa
    // Conti-mer chains (one per contig placement): following `next` from a conti-mer never looks at mutable state
    // (AG:2064-2072), so the walk appends a precomputed suffix instead of chasing pointers.  Built by build_chains().
    std::vector<size_t> chain_off;          // [n_chains+1] chain c's bases are chain_str[chain_off[c] .. chain_off[c+1])
    std::vector<agx_u32> chain_end_pos;     // position of the chain's terminal conti-mer
    std::string chain_str;
    // per-position hop table (agx_hop, agx_core.h)
    std::vector<agx_hop> hop;               // [n_pos]
    // the same chains as runs (agx_cmseg): what the device gets instead of cm_start / cm / hop.  The first n_seg0 are the rank-0 runs, by position.
    std::vector<agx_cmseg> segs; agx_u32 n_seg0 = 0;
};
void build_chains(Threads &T);

// Packed read alignments of one unit (loadSeq/loadReadAli, AG:361-404, 1233-1277)
struct Pairs {
    std::vector<agx_hit> hits;             // processing order
    std::vector<agx_run> runs;
    std::string bases;                     // read slot s occupies [s*stride, s*stride+len)
    agx_u32 stride = 0;
    agx_u32 n_slots = 0;
    unsigned long long n_pairs_in_file = 0, n_sam_pairs = 0, n_kept = 0;
};

// What the host walk (and the engine's staging) reads of a loaded unit, wherever it lives: in the loader's containers (Threads / Pairs) or in
// a mapped unit cache file (agx_engine.cpp).
struct UnitView {
    const char *ref = nullptr; size_t n_pos = 0; agx_u32 n_ref = 0;   // unit sequence + appended positions
    const agx_u32 *cm_start = nullptr;                                // [n_pos + 1], or null: then cm_cnt
    const agx_u8 *cm_cnt = nullptr;                                   // [n_pos] conti-mers per position (the fast loader and the unit cache keep counts, not a prefix)
    const char *chain_str = nullptr;                                  // conti-mer chain suffixes (agx_hop::str_off points in here)
    const agx_hop *hop = nullptr;                                     // per-position hop table, or null: then GraphView::sp_hop, and for ids outside it the runs below
    const agx_cmseg *segs = nullptr; agx_u32 n_seg0 = 0;              // the conti-mer chains as runs (rank-0 runs first, by position): hop entries by bisection (agx_seg_hop)
    const char *bases = nullptr; agx_u32 stride = 0;                  // read bases, slot s at bases + s * stride (k-mer strings of written records)
    const uint64_t *row_off = nullptr;                                // or: row r of the staged read bases starts at bases + row_off[r] (the mapped reads file; GraphView::row_slot is then not consulted)
    // or (bases == nullptr): the k-mer tails come out of the staged 2-bit rows themselves — row r = codes2 + r * (stride / 4), base j in bits 2 * (j & 3) of byte j >> 2 (agx_pack_classes2) —
    // and the list of the bases that are not A, C, G, T (index r * stride + j, ascending) with their bytes.  Units whose read alignments were handed over staged (tmp/_agx_pairs.<u>.bin) have
    // nothing else; the arrays live in the mapped file (the pinned copies are gone once a one-shot unit has been downloaded).
    const agx_u8 *codes2 = nullptr; const unsigned long long *other_idx = nullptr; const agx_u8 *other_byte = nullptr; size_t n_other = 0;
    // r06, tile-ordered upload: the device numbers the read rows by the hit's place in the tile order (every hit's left-mate row travels at that place); slot_row[place] = the row
    // of the staged arrays above (null: the k-mer string references name those rows themselves)
    const agx_u32 *slot_row = nullptr;
    bool has_cm(size_t x) const { return cm_cnt ? cm_cnt[x] != 0 : cm_start[x + 1] > cm_start[x]; }
    agx_u32 cm_count(size_t x) const { return cm_cnt ? cm_cnt[x] : cm_start[x + 1] - cm_start[x]; }
    const char *initial = nullptr; size_t n_initial = 0;              // bytes of tmp/_initial_contigs.<u>.fa
};
inline UnitView view_of(const Threads &T, const Pairs &P) {
    UnitView V; V.ref = T.ref.data(); V.n_pos = T.ref.size(); V.n_ref = T.n_ref; V.cm_start = T.cm_start.size() == T.ref.size() + 1 ? T.cm_start.data() : nullptr;
    V.cm_cnt = T.cm_cnt.size() == T.ref.size() ? T.cm_cnt.data() : nullptr; V.chain_str = T.chain_str.data();
    V.hop = T.hop.size() == T.ref.size() ? T.hop.data() : nullptr; V.segs = T.segs.data(); V.n_seg0 = T.n_seg0; V.bases = P.bases.data(); V.stride = P.stride; V.initial = T.initial_contigs.data(); V.n_initial = T.initial_contigs.size();
    return V;
}

// Walk graph as downloaded from the device (or produced by the test executor); see agx_core.h "walk preparation".
// Walk ids: [0, n_pos) = first alive variant of each position (AGX_WM_ABSENT where there is none), [n_pos, n_ids) = further variants.
// Node records come as the sparse table of the special ids; any other id (only reachable after the +1000 skip) goes through fetch().
struct GraphView {
    agx_u32 n_pos = 0, n_ids = 0;
    const agx_u8 *meta = nullptr;                           // [n_ids + 64] AGX_WM_* bits (padding reads as 0)
    agx_u8 *meta_rw = nullptr;                              // null, or == meta: the walk may keep its visited marks in meta's bit 7 (the array is consumed by the walk)
    enum { MAX_WALKERS = 16 };                              // a large unit is walked by several walkers (agx_walk.cpp: walk_split), each of the further ones on a window of meta that it copies for itself
    const char *str = nullptr;                              // [n_ids] base a node emits
    const agx_u32 *side_xpos = nullptr;                     // [n_ids - n_pos] position of each side id, non-decreasing
    const unsigned long long *sp_bits = nullptr;            // [n_ids/64 + 1] special-id bitmap
    const agx_u32 *sp_rank = nullptr;                       // [n_ids/64 + 1] special ids before each 64-id word
    const agx_walknode *sp_node = nullptr; agx_u32 n_special = 0;   // records of the special ids, id order
    const agx_hop *sp_hop = nullptr;                        // [n_special] hop entry of each special id's position (optional: else UnitView::hop)
    // records of non-special ids: `rows` groups of `width` consecutive ids, group r starting at first + r*stride, into out[rows*width]
    void (*fetch)(void *ctx, agx_u32 first, agx_u32 stride, agx_u32 rows, agx_u32 width, agx_walknode *out) = nullptr; void *fetch_ctx = nullptr;
    const agx_edge_ovf *ovf = nullptr; size_t n_ovf = 0;     // walk ids; NONE/NONE entries and duplicates are ignored
    const agx_u32 *row_slot = nullptr;                      // k-mer string references name rows of the staged read bases: row -> read slot (null: they name read slots)
    // Streamed download (r06; agx_engine.cpp: begin_streamed_download): meta, sp_bits, sp_rank, sp_node and sp_hop fill in behind the walk's back, a position window at a
    // time from the front — main ids [0, x) together with the side ids of the positions below x —, str last; side_xpos and ovf are in place from the start.
    // wait_landed returns when everything about main ids [0, main_hi) and side ids [n_pos, side_hi) is in place; wait_str when str is.  The walk never looks at a byte it has
    // not waited for: the further walkers of walk_split wait for their windows and are confined to them (as they always were), the first walker — the only one whose walks may lead
    // anywhere — waits for everything and gets the shortest stretch in exchange (land_ms: what is left of the download when the walk begins, for that balance).
    void (*wait_landed)(void *ctx, agx_u32 main_hi, agx_u32 side_hi) = nullptr; void (*wait_str)(void *ctx) = nullptr; void *land_ctx = nullptr; double land_ms = 0;
};

// Megabyte-sized buffers that are written once, front to back (outputs, the walk's visited bytes): ask for transparent huge pages where
// the kernel offers them on request (THP "madvise" mode), so first-touch costs a few faults instead of one per 4 KB.  Advisory only.
void advise_huge(void *p, size_t n);

// malloc-backed output buffer whose storage can be handed to the C caller without another copy
// Output buffers that were handed to a caller and given back (agx_result_free) are kept for the next unit instead of going back to the C library: a unit's three outputs
// are 2.2 bytes per position of FRESH memory otherwise — page faults and the kernel's zeroing, a sixth of a whole-human job's host CPU time (r05) — and a run's units
// follow each other.  malloc'd memory throughout (a caller may free() an output itself); at most 128 buffers / 16 GB are kept (a whole-human job's 24 units hand back 72 buffers, 6.8 GB); agx_pool_trim(-1) frees them.
void *out_cache_take(size_t need, size_t &cap);      // a kept buffer of at least `need` bytes and at most twice that (cap = its usable size); nullptr: none
void out_cache_give(void *p);                        // (nullptr is fine)
void out_cache_trim();
struct OutBuf {
    char *p = nullptr; size_t n = 0, cap = 0;
    OutBuf() = default; OutBuf(const OutBuf &) = delete; OutBuf &operator=(const OutBuf &) = delete;
    ~OutBuf() { out_cache_give(p); }
    void reserve(size_t c) {
        if (c + 1 <= cap) return;
        if (!p && c >= ((size_t)1 << 20)) { size_t got = 0; if (void *q = out_cache_take(c + 1, got)) { p = (char *)q; cap = got; return; } }
        char *q = (char *)realloc(p, c + 1); if (!q) throw Error{E_ARG, "out of host memory"};
        p = q; cap = c + 1; advise_huge(p, cap);
    }
    char *grow(size_t add) { if (n + add + 1 > cap) reserve((n + add) + (n + add) / 2 + 64); char *w = p + n; n += add; return w; }
    void append(const char *s, size_t len) { memcpy(grow(len), s, len); }
    char *release() { if (!p) reserve(0); p[n] = 0; char *r = p; p = nullptr; n = cap = 0; return r; }
    // touches every page of the capacity: the first-touch faults (and the kernel's zeroing) of a 30 MB output happen where the caller has
    // time to spare instead of inside the walk
    void prefault() { for (size_t i = 0; i < cap; i += 4096) p[i] = 0; }
    void clear() { out_cache_give(p); p = nullptr; n = cap = 0; }
};
// The graph stretches of the written pre-extended records (agx_unit_walk_paths, include/agx.h: agx_walk_paths): per record its bases and the end of its stretches, per
// stretch the walk ids, where its bases begin in the record, and whether it continues the stretch in front of it over an edge
struct WalkPaths {
    std::vector<uint64_t> rec_len, st_end, base_off; std::vector<agx_u32> id_first, id_last; std::vector<agx_u8> joined;
    void clear() { rec_len.clear(); st_end.clear(); base_off.clear(); id_first.clear(); id_last.clear(); joined.clear(); }
};
struct UnitOutput { OutBuf pre_extended, extended; unsigned long long n_fetched = 0;
                    bool keep_paths = false, paths_ready = false; WalkPaths paths; };      // keep_paths: the walk fills `paths` (AGX_FLAG_KEEP_PATHS); else it is not touched

// read-only view of a whole file (mmap)
struct FileView {
    const char *p = nullptr; size_t n = 0; int fd = -1; bool mapped = false;
    explicit FileView(const std::string &path);
    ~FileView();
    FileView(const FileView &) = delete; FileView &operator=(const FileView &) = delete;
};

// Threads of a loader: `threads` workers that live as long as the team and run one function after another (a phase of a loader = one run()).
// Nothing leaves a worker as an exception: what one throws is rethrown by run() on the caller's thread.
class Team {
public:
    explicit Team(unsigned threads);
    ~Team();
    unsigned size() const { return n_; }
    void run(const std::function<void(unsigned)> &fn);      // fn(t) for t in [0, size()), t = 0 on the calling thread
private:
    struct Impl; Impl *impl_; unsigned n_;
};
// Scratch memory of the loaders: anonymous mappings, huge pages asked for, kept in a process-wide cache when they are given back (a unit's
// loader touches as much temporary memory as it produces output; fresh 4 KB pages cost it more than the parsing itself, and 160 threads faulting
// them in at once wait for each other on the address-space lock — the next unit finds the pages of the last one already there).
struct Scratch {
    void *p = nullptr; size_t n = 0;
    Scratch() = default; explicit Scratch(size_t bytes) { take(bytes); }
    ~Scratch() { give(); }
    Scratch(const Scratch &) = delete; Scratch &operator=(const Scratch &) = delete;
    Scratch(Scratch &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    Scratch &operator=(Scratch &&o) noexcept { if (this != &o) { give(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    void take(size_t bytes); void give();
};
void scratch_trim();      // unmaps what the cache holds
// fixed-capacity array in scratch memory (the capacity is an upper bound known before the fill; grow() for the rare case that it was a guess)
template <class T> struct SBuf {
    Scratch s; T *p = nullptr; size_t n = 0, cap = 0;
    SBuf() = default;
    SBuf(SBuf &&o) noexcept : s(std::move(o.s)), p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    SBuf &operator=(SBuf &&o) noexcept { if (this != &o) { s = std::move(o.s); p = o.p; n = o.n; cap = o.cap; o.p = nullptr; o.n = o.cap = 0; } return *this; }
    void reserve(size_t c) { if (c <= cap) return; Scratch m(c * sizeof(T) + 64); if (n) memcpy(m.p, p, n * sizeof(T)); s = std::move(m); p = (T *)s.p; cap = c; }
    void push_back(const T &v) { if (n == cap) reserve(cap ? cap * 2 : 1024); p[n++] = v; }
    void append(const T *src, size_t k) { if (n + k > cap) reserve(std::max(cap * 2, n + k)); memcpy(p + n, src, k * sizeof(T)); n += k; }
    T &operator[](size_t i) { return p[i]; } const T &operator[](size_t i) const { return p[i]; }
    T &back() { return p[n - 1]; } const T &back() const { return p[n - 1]; } size_t size() const { return n; } bool empty() const { return n == 0; } void resize_down(size_t k) { n = k; }
    T *begin() { return p; } T *end() { return p + n; } const T *begin() const { return p; } const T *end() const { return p + n; } T *data() { return p; } const T *data() const { return p; }
};

unsigned cgroup_cpu_quota(const char *proc_cgroup, const char *sys_root);   // tightest CPU quota over the process's control groups (v1 and v2, nested), 0 = none
unsigned usable_cpus();                   // CPUs this process can keep busy: its affinity mask capped by the CPU quota of its control group
unsigned loader_threads(size_t bytes);      // AGX_LOAD_THREADS, else by the size of the input and the cores this process may use
// walkers of a unit of n positions at most (agx_walk.cpp: walk_split): AGX_WALK_SPLIT_WALKERS (two to sixteen), else one per 1.2 M positions, two to eight.  The engine hands
// out one per CPU this process may use at most (agx_engine.cpp: walkers_now).
inline thread_local int walkers_cap = 8;      // set by the engine for the walk that begins on this thread: sixteen when no other unit is on its way (the tail of a job), else eight
inline int walkers_for(size_t n) {
    const char *e = getenv("AGX_WALK_SPLIT_WALKERS");
    // (r04: eight by default, sixteen on request.  Measured on the cfg3 job: 35.43 ms and 386 CPU-ms per job with up to sixteen, 35.58 ms and 299 CPU-ms with eight, 38.98 ms with
    // four — every walker beyond what the walk's length needs is a window copy, a warm-up and a thread that spins up for nothing)
    const int k = e ? atoi(e) : (int)std::min<size_t>(n / 1200000u, (size_t)walkers_cap);
    return k < 2 ? 2 : k > GraphView::MAX_WALKERS ? (int)GraphView::MAX_WALKERS : k;
}

// agx_load.cpp — the fast loaders.  Each returns false when the input is anything but the well-formed common case (an '@' line, an empty line in the
// middle, ids out of order, blocks that overlap, whatever would be an error): the caller then takes the general loader of agx_host.cpp, which follows
// the reference line by line and reports errors in its order.  What they return is byte for byte what the general loader + staging produce.
struct ReadsIndex;
enum { SA_HITS = 0, SA_SIDES, SA_RUNS, SA_CODES, SA_OTHER, SA_JUMP, SA_N };
struct StageSink { virtual void *take(int which, size_t bytes) = 0; virtual ~StageSink() {} };      // where the staged arrays live (the engine: pinned memory)
struct StagedPairs {        // what the upload wants of a unit's read alignments, in the wire formats of agx_core.h (agx_engine.cpp: staging; their upload forms: agx_forms.h)
    agx_whit *hits = nullptr; size_t nh = 0;             // row = ROW of the left mate's bases, AGX_WF_LEFT2 = which mate that is
    agx_wside *sides = nullptr; size_t n_sides = 0;      // one per hit with a multi-run mate
    agx_wrun *runs = nullptr; size_t n_runs = 0;
    agx_u8 *codes = nullptr; size_t n_codes = 0;         // 2-bit classes, stride / 4 bytes per row
    unsigned long long *other = nullptr; size_t n_other = 0;   // bases that are not A, C, G, T: row * stride + index, ascending
    agx_u32 *jump = nullptr; size_t n_jump = 0;          // the hits whose LEFT mate has two or more runs, ascending: the only ones pass J of the edge build has to look at (agx_edge_jump_hit)
    agx_u32 stride = 0, maxlen = 0, n_rows = 0;          // stride: bases per row = the longest read rounded up to 4
    std::vector<uint64_t> row_off;                       // fast loader: where each row's bases start in the reads file
    std::vector<agx_u32> row_slot;                       // general loader: the read slot (Pairs::bases) of each row
    unsigned long long n_pairs_in_file = 0, n_sam_pairs = 0;
};
bool thread_contigs_fast(const std::string &contigs_fa, const std::string &psl, Threads &T);      // T.ref must hold the unit sequence (left as it was on false)
bool load_pairs_fast(const ReadsIndex &reads, const std::string &sam, long batch, agx_u32 k, unsigned threads, StageSink &sink, StagedPairs &S);
// the same arrays from what the general loader (or agx_unit_push_pairs) holds; staged_out (tests): the hits as the device will unpack them
void stage_pairs(const Pairs &P, agx_u32 k, unsigned threads, StageSink &sink, StagedPairs &S, std::vector<agx_hit> *staged_out = nullptr);
// The staged hits in the order of the tile their first arrival falls in (agx_core.h "hits in tile order"): perm[i] = the i-th hit of that order (hit numbers ascend inside a
// tile), tile_first[t] = hits in front of tile t's own (n_tiles + 2 entries, the last two = nh), jump_at = pass J's list (`jump`, hit numbers) as places in the order, ascending
void order_hits(const agx_whit *hits, size_t nh, const agx_wside *sides, const agx_wrun *runs, const agx_u32 *jump, size_t n_jump, size_t n_pos, unsigned threads,
                agx_u32 *perm, agx_u32 *tile_first, agx_u32 *jump_at);
// reference bases as 2 bits each + the stretches of other bytes (agx_core.h); false: too many such stretches (soft-masked sequence): the bases cross as they are
// what the device builds the conti-mer tables from besides the runs themselves (agx_core.h: agx_cntrun, agx_chunk): the counts as runs, and both run lists in chunks
struct CmLayout { std::vector<agx_cntrun> cnt_runs; std::vector<agx_chunk> cnt_chunks, seg_chunks; std::vector<agx_u32> seg_index; };
void build_seg_index(const agx_cmseg *segs, size_t n_seg0, size_t n_pos, std::vector<agx_u32> &index);      // agx_compact_args::seg_index
void build_cm_layout(const agx_u8 *cm_cnt, size_t n_pos, const agx_cmseg *segs, size_t n_segs, CmLayout &L);      // (seg_index is built separately: it needs n_seg0)
bool pack_reference(const char *ref, size_t n, unsigned threads, agx_u8 *packed /* (n + 3) / 4 + 16 bytes */, std::vector<agx_refx> &others);
// The read rows in their upload form (agx_core.h "read rows relative to the reference").  cnt: one count byte per row, padded with zeros to whole 64-row blocks + 64;
// block_off[i]: units in front of row 64 i (and the total behind the last block); anchor_bits: bit h = hit h is its row's anchor; units: the stream.
// block_first[i]: the anchor of row 64 i.
struct RowDiffs { std::vector<agx_u8> cnt; std::vector<agx_u32> block_off, block_first, anchor_bits; std::vector<agx_u16> units; size_t n_units = 0, n_explicit = 0; };
// wref: the packed reference (pack_reference) as 32-bit words, readable one word beyond position n_pos + 15.  false: the form does not apply.
bool build_row_diffs(const agx_whit *hits, size_t nh, const agx_wside *sides, size_t n_sides, const agx_wrun *runs, size_t n_runs, const agx_u8 *codes2, size_t n_rows, agx_u32 stride,
                     const agx_u32 *wref, size_t n_pos, unsigned threads, RowDiffs &D, bool rows_are_hits = false);

// tmp/_agx_pairs.<u>.bin — a unit's read alignments handed over STAGED (the wire formats of agx_core.h) instead of as SAM text + tmp/_reads.fa: what an aligner that is
// linked with the engine (or a generator of synthetic alignments: tools/agx_synth.cpp) writes where the reference's flow distributes SAM lines (AG:3545-3579).  The arrays are
// exactly what the loaders + staging produce from the text (tests/test_staged_pairs.py compares them byte for byte); they depend on k (which mate is the left one) and on
// BATCH (which line pairs the batch boundaries drop), both in the header.  agx_unit_load_files takes the file when it is there and does not look for the two text files.
// The format's contract for a producer outside this tree — what the loader holds a file to besides the header's lengths (rule names as staged_pairs_rule returns them;
// a file that breaks one is refused with AGX_E_FORMAT and the name):
//   hit_row, hit_len    row < n_rows; 0 < len <= maxlen
//   hit_back            back <= the hit's own number (the earlier hits of its pair)
//   hit_flags           only the five bits REV1, REV2, LEFT2, RUNS1, RUNS2 (AGX_WF_DUP is the staging's)
//   hit_side, side_runs a hit with RUNS1 / RUNS2 names a side record < n_sides in a (RUNS1) or b (RUNS2 only); a side's runs lie inside the pool: runs + nruns <= n_runs
//   run_in_read         every run lies in its read: q + n <= len
//   run_order           a mate's runs ascend and do not overlap, in the read and on the reference: q + n <= next q, t + n <= next t
//   mate_in_unit        every aligned base of the mate that is NOT the left one lies inside the unit sequence (position + len, or t + n of each run, <= its length
//                       with the positions contig threading appends); the left mate's span is checked on the device
//   jump_*              S_JUMP lists exactly the hits whose LEFT mate has two runs or more: as many (jump_count), each < nh (jump_entry), ascending (jump_order), each one of them (jump_hit)
//   other_in_rows, other_order   S_OTHER entries < n_rows * stride, strictly ascending; S_OTHERB[i] is the byte of entry i
namespace pairsfile {
enum { S_HITS = 0, S_SIDES, S_RUNS, S_CODES, S_OTHER, S_OTHERB, S_JUMP, S_N };
struct Header {
    char magic[8]; agx_u32 version, k, batch, stride, maxlen, n_rows;
    unsigned long long nh, n_sides, n_runs, n_codes, n_other, n_jump, pairs_in_file, sam_pairs;
    agx_u32 sizes[3];                            // sizeof agx_whit, agx_wside, agx_wrun
    unsigned long long off[S_N], len[S_N];
};
const char MAGIC[8] = {'A', 'G', 'X', 'P', 'A', 'I', 'R', '1'};
inline std::string path_of(const std::string &dir, int unit) { return dir + "/_agx_pairs." + std::to_string(unit) + ".bin"; }
}  // namespace pairsfile
// other_bytes[i] = the byte of listed base i (S.other[i]).  Throws Error{E_IO} if the file cannot be written.
void write_pairs_file(const std::string &path, const StagedPairs &S, const agx_u8 *other_bytes, agx_u32 k, agx_u32 batch);
std::vector<agx_u8> other_bytes_of(const Pairs &P, const StagedPairs &S);      // from the general loader's containers (S.row_slot names P's read slots)
// maps and checks the header and the section lengths (not the content); false: no such file.  Throws Error{E_FORMAT} on a file that is not one.
struct PairsFile { std::unique_ptr<FileView> fv; pairsfile::Header H; const char *sec(int i) const { return fv->p + H.off[i]; } };
bool open_pairs_file(const std::string &path, PairsFile &F);

// tmp/_agx_unit.<u>.bin — a unit's STAGED form (agx_engine.cpp "unit cache file" writes and loads it): its header and section numbers, here so that host-only code can
// judge a header and a file's content without a device.
namespace cachefile {
enum { S_HITS = 0, S_RUNS, S_CODES, S_SEGS, S_CHAIN_END, S_ROWS, S_REF, S_CM_CNT, S_CHAIN_STR, S_INITIAL, S_BASES, S_OTHER, S_SIDES, S_JUMP, S_OTHERB, S_N };
struct Header {
    char magic[8]; agx_u32 version, batch; unsigned long long stamp[6][2];      // (size, modification time) of the five text files and of tmp/_agx_pairs.<u>.bin
    unsigned long long n_pos, n_ref, nh, n_runs, n_cm, n_segs, n_seg0, n_rows, n_chain_end, n_codes, pairs_in_file, sam_pairs;
    agx_u32 stride, maxlen, n_slots, k;          // k: the staged hits name their left mate, which depends on it (agx_hit_left_is_mate2)
    agx_u32 rows_in_reads;                       // 1: S_ROWS holds 64-bit offsets into tmp/_reads.fa (whose size and time are part of the stamp), S_BASES is empty; 0: S_ROWS holds the
                                                 // read slot of every row and S_BASES the slots' bases (units that the general loader parsed); 2: both empty — the k-mer tails come out of
                                                 // S_CODES (2-bit rows) and S_OTHER / S_OTHERB (units whose alignments were handed over staged: UnitView::codes2)
    agx_u32 slot_stride;                         // bases per read slot in S_BASES (rows_in_reads == 0)
    unsigned long long n_sides, n_jump;
    agx_u32 sizes[5];                            // sizeof agx_whit, agx_wrun, agx_cmseg, Header, agx_wside: a file written by another layout is not this one
    unsigned long long off[S_N], len[S_N];
};
const char MAGIC[8] = {'A', 'G', 'X', 'U', 'N', 'I', 'T', '7'};
}  // namespace cachefile

// ---- what a staged-pairs file and a unit cache file must hold besides intact lengths (agx_load.cpp "content rules") ----
// Everything the device and the walk index with must be in range: a file whose lengths are intact but whose content is not is a reason to refuse it, not to read out of
// bounds.  Each check returns the NAME of the first rule that fails (short, stable: DESIGN.md "Rejected inputs" lists them with what each protects), or nullptr.
// The staged read alignments, as both files hold them.  n_pos: the unit's positions, 0 where they are not known yet (the rules that need them are then left out:
// staged_positions_rule applies them alone, later).
struct StagedView {
    const agx_whit *hits = nullptr; size_t nh = 0; const agx_wside *sides = nullptr; size_t n_sides = 0; const agx_wrun *runs = nullptr; size_t n_runs = 0;
    const agx_u32 *jump = nullptr; size_t n_jump = 0; const unsigned long long *other = nullptr; size_t n_other = 0;
    unsigned long long n_rows = 0; agx_u32 stride = 0, maxlen = 0; unsigned long long n_pos = 0;
};
const char *staged_pairs_rule(const StagedView &V, unsigned threads);
const char *staged_positions_rule(const StagedView &V, unsigned threads);      // the rules of staged_pairs_rule that need V.n_pos, alone
const char *other_ascending_rule(const unsigned long long *other, size_t n_other);      // the walk bisects the list (where it reads k-mer tails out of the 2-bit rows)
// the header of a staged-pairs file of `file_size` bytes (open_pairs_file)
const char *pairs_header_rule(const pairsfile::Header &H, unsigned long long file_size);
const char *pairs_unit_rule(const pairsfile::Header &H, agx_u32 k, agx_u32 batch);      // the file was staged for this unit's k and BATCH
// the header of a cache file of `file_size` bytes, for a unit of this BATCH and k (not the stamps: they are compared with the files beside it)
const char *cache_header_rule(const cachefile::Header &H, unsigned long long file_size, agx_u32 batch, agx_u32 k);
// what a cache file holds besides the staged read alignments: the conti-mer runs, the counts they fill, the chain ends, the rows' places.  reads_size: bytes of tmp/_reads.fa
// (rows_in_reads == 1); rows: section S_ROWS
struct CacheView {
    const agx_cmseg *segs = nullptr; size_t n_segs = 0; const agx_u8 *cm_cnt = nullptr; const agx_u32 *chain_end = nullptr; size_t n_chain_end = 0; const void *rows = nullptr;
    unsigned long long n_pos = 0, n_cm = 0, n_rows = 0, chain_str_len = 0, reads_size = 0; agx_u32 maxlen = 0, n_slots = 0, rows_in_reads = 0;
};
const char *cache_content_rule(const CacheView &C, unsigned threads);
const char *const *content_rule_names(size_t *n);      // every name the checks above can return

// agx_host.cpp
void load_unit_reference(const std::string &path, std::string &ref);
void thread_contigs_from_files(const std::string &contigs_fa, const std::string &psl, Threads &T);   // T.ref must hold the unit sequence
// tmp/_reads.fa mapped once with the byte offset of every record: the units of one run (AG:1880 re-reads the whole file for each of
// them) then only touch the reads their own SAM names.  Immutable after open(); shared by any number of threads.
struct ReadsIndex {
    FileView fv;
    SBuf<uint64_t> rec_off;                     // offset of the first line of record r (a record = two lines)
    unsigned long long headers = 0;             // header lines up to the first empty line
    explicit ReadsIndex(const std::string &path);
};
ReadsIndex *reads_index_open(const std::string &reads_fa);
void reads_index_close(ReadsIndex *);
// reads: optional index of reads_fa (nullptr: the file is scanned here)
void load_pairs_from_files(const std::string &reads_fa, const std::string &sam, long batch, agx_u32 k, Pairs &P, const ReadsIndex *reads = nullptr);

// agx_walk.cpp
// A second thread the walk may hand work to (the engine: the unit's helper thread): run(f) starts f there, wait() returns when it is done.
// The walk itself is sequential by specification; copying the written records' bases into the outputs is not.
struct Assistant {          // (helpers(): how many threads there are; `who` picks one)
    virtual void run(std::function<void()> f, int who = 0) = 0; virtual void wait(int who = 0) = 0; virtual int helpers() const { return 1; } virtual ~Assistant() {}
};
void walk_join_scaffold(const UnitView &V, const GraphView &G, UnitOutput &out, Assistant *assistant = nullptr);

// The jump table of agx_unit_walk_span (host only, here so that the engine and the tests' serial replay run the same function): the n jumps of a chunk as
// the device listed them (positions x < y, flat base) sorted by (x, y, base) and merged into entries, one per distinct (x, y), in the form agx_k_sp_jumps and
// agx_k_sp_scatter read: e_x / e_y per entry, and per jump its base and its entry.  false: a listed jump is not forward (the device's list is inconsistent).
struct SpanJumps { std::vector<agx_u32> e_x, e_y, l_base, l_ent; };
inline bool span_jump_entries(const agx_u32 *x, const agx_u32 *y, const agx_u32 *base, size_t n, SpanJumps &J) {
    J.e_x.clear(); J.e_y.clear(); J.l_base.assign(n, 0); J.l_ent.assign(n, 0);
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) { if (y[i] <= x[i]) return false; order[i] = i; }
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return x[a] != x[b] ? x[a] < x[b] : y[a] != y[b] ? y[a] < y[b] : base[a] < base[b]; });
    for (size_t k = 0; k < n; k++) {
        const size_t i = order[k];
        if (J.e_x.empty() || J.e_x.back() != x[i] || J.e_y.back() != y[i]) { J.e_x.push_back(x[i]); J.e_y.push_back(y[i]); }
        J.l_base[k] = base[i]; J.l_ent[k] = (agx_u32)(J.e_x.size() - 1);
    }
    return true;
}

// The passes of agx_unit_mate_links (host only, here so that the engine and the tests' serial replay run the same function).  pass(a_lo, a_hi, first) runs one
// pass over all hits for the links whose left record lies in [a_lo, a_hi) and says whether every pair found a slot; a pass that did not is discarded by its caller and its
// range halved.  The ranges that fit come in ascending order and are disjoint.  Returns the passes run, or -1 with *stuck the record whose links alone do not fit the table.
template <class PASS>
inline long links_plan(agx_u32 n_recs, PASS pass, agx_u32 *stuck) {
    std::vector<std::pair<agx_u32, agx_u32>> todo{{0u, n_recs}};
    long passes = 0;
    while (!todo.empty()) {
        const std::pair<agx_u32, agx_u32> r = todo.back();
        todo.pop_back();
        const bool fit = pass(r.first, r.second, passes == 0);
        passes++;
        if (fit) continue;
        if (r.second - r.first <= 1u) { *stuck = r.first; return -1; }
        const agx_u32 mid = r.first + (r.second - r.first) / 2u;
        todo.push_back({mid, r.second}); todo.push_back({r.first, mid});
    }
    return passes;
}

}  // namespace agx
