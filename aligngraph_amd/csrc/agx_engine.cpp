// agx_engine.cpp — device memory, kernel sequencing and the C-ABI of libagx.so (include/agx.h) from a unit's creation to its finish, with the calls that copy build state
// out.  The unit object itself is agx_unit.h; the calls that answer a question about a built unit out of the export's scratch are agx_export.cpp.
//
// One agx_unit = one reference unit (chromosome or --part slice) = the body of the reference's unit loop
// (AG:4765-4783).  In the application every unit is NEW data and is built once, so what a unit costs is the whole way
// from its packed arrays in host memory to its output bytes in host memory (SURVEY §8d's T_core):
//   stage    (when the arrays are handed over, outside T_core) the arrays the device wants are packed into pinned memory: hits and runs
//            as they are, the read bases as 4-bit classes, the conti-mer keys without the walk's fields;
//   upload   one block of HBM for everything the unit will ever hold (agx_mem.h), asynchronous copies at PCIe rate on the unit's own
//            stream — beside other units' kernels —, two small kernels (conti-mer heads, vote codes), an event;
//   build    all kernels queued back to back on the device's two build streams behind that event, ONE synchronisation, capacities
//            chosen so that a first build does not have to be repeated;
//   download the walk graph into cached pinned buffers; finish = the sequential host walk.
// No CPU fallback exists: a host without a HIP device gets AGX_E_NOGPU from agx_unit_create.
#include "agx_unit.h"


// Downloads through the HSA runtime's asynchronous copy, i.e. the SDMA engines.  hipMemcpyAsync does a device-to-host copy into registered
// memory with a copy KERNEL of its own (rocprofv3: __amd_rocclr_copyBuffer), and a kernel that stores to host memory slows what runs beside
// it — under rocprofv3 the next unit's agx_k_tile_sort ran 2.6-4.2 ms instead of 0.8 and the device window of a cfg3 job was 49 ms instead of
// 42 (profiles/r02_f_timeline.txt vs r02_g_timeline.txt; un-profiled the job takes the same 59 ms either way: the builds are not what the
// last walks wait for).  The engines move the same bytes at the same 56 GB/s (tests/tools/sdma_d2h.cpp) and leave the CUs alone.  Set up
// once per process; if anything about it fails (AGX_NO_SDMA_DOWNLOAD forces that) the copies go through HIP.
struct HsaCopy {
    bool ok = false; hsa_agent_t cpu{}; std::vector<hsa_agent_t> gpu; std::vector<std::string> uuid;      // uuid: "GPU-<16 hex digits>" of each GPU agent
    static hsa_status_t on_agent(hsa_agent_t a, void *p) {
        HsaCopy *H = (HsaCopy *)p; hsa_device_type_t t;
        if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
        if (t == HSA_DEVICE_TYPE_CPU && !H->cpu.handle) H->cpu = a;
        if (t == HSA_DEVICE_TYPE_GPU) {
            char id[32] = {0};
            (void)hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_UUID, id);
            H->gpu.push_back(a); H->uuid.push_back(std::string(id, strnlen(id, 21)));
        }
        return HSA_STATUS_SUCCESS;
    }
    HsaCopy() {
        if (getenv("AGX_NO_SDMA_DOWNLOAD")) return;
        if (hsa_init() != HSA_STATUS_SUCCESS) return;
        if (hsa_iterate_agents(on_agent, this) != HSA_STATUS_SUCCESS) return;
        ok = cpu.handle != 0 && !gpu.empty();
    }
    // the agent of HIP device `device`, by its UUID (the two runtimes need not number the devices alike, and report different PCI
    // addresses inside a container); one device on either side is that device; false: not found
    bool agent_of(int device, hsa_agent_t &out) const {
        static std::mutex m; static int known[64]; static hsa_agent_t agent[64];      // known: 0 not asked yet, 1 found, -1 not found
        std::lock_guard<std::mutex> l(m);
        int &k = known[device & 63];
        if (!k) {
            k = -1;
            hipDeviceProp_t prop;
            if (ok && hipGetDeviceProperties(&prop, device) == hipSuccess) {
                const std::string want = "GPU-" + std::string(prop.uuid.bytes, strnlen(prop.uuid.bytes, 16));
                int n_hip = 0;
                for (size_t i = 0; i < gpu.size(); i++) if (uuid[i] == want && want.size() > 4) { agent[device & 63] = gpu[i]; k = 1; break; }
                if (k != 1 && gpu.size() == 1 && hipGetDeviceCount(&n_hip) == hipSuccess && n_hip == 1) { agent[device & 63] = gpu[0]; k = 1; }
            }
        }
        if (k == 1) out = agent[device & 63];
        return k == 1;
    }
};
const HsaCopy &hsa_copy() { static const HsaCopy h; return h; }

// positions from which a unit's host walk is split between two walkers (= walk_split's default in agx_walk.cpp; AGX_WALK_SPLIT_MIN, read at every download, overrides both: tests)
inline size_t two_walkers_min() { const char *e = getenv("AGX_WALK_SPLIT_MIN"); return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)4000000; }
#define AGX_TWO_WALKERS_MIN two_walkers_min()
// walkers for a unit of n_pos positions (walkers_for, agx_host.h)
inline int walkers_wanted(size_t n_pos) { return n_pos < AGX_TWO_WALKERS_MIN ? 1 : walkers_for(n_pos); }


// The further walkers of large units (agx_walk.cpp: walk_split; the first extra one is the unit's own helper): a small pool for the process, made
// when the first large unit is finished.  A unit takes what is free and walks with fewer walkers if that is less than it wanted.
struct WalkerPool {
    enum { N = 64 };
    struct Slot { std::thread th; std::mutex m; std::condition_variable cv; std::function<void()> job; bool queued = false, running = false, taken = false, stop = false; };
    Slot slot[N]; std::mutex take_m; bool started = false;
    void start() {
        if (started) return;
        started = true;
        for (Slot &s : slot) {
            try {
                s.th = std::thread([&s] {
                    pthread_setname_np(pthread_self(), "agx-walker");
                    std::unique_lock<std::mutex> l(s.m);
                    for (;;) {
                        s.cv.wait(l, [&s] { return s.stop || s.queued; });
                        if (s.stop) return;
                        std::function<void()> f = std::move(s.job); s.queued = false; s.running = true;
                        l.unlock();
                        try { f(); } catch (...) { }
                        l.lock(); s.running = false; s.cv.notify_all();
                    }
                });
            } catch (...) { s.taken = true; }        // (never handed out)
        }
    }
    int take() { std::lock_guard<std::mutex> l(take_m); start(); for (int i = 0; i < N; i++) if (!slot[i].taken) { slot[i].taken = true; return i; } return -1; }
    void give(int i) { std::lock_guard<std::mutex> l(take_m); slot[i].taken = false; }
    void run(int i, std::function<void()> f) { Slot &s = slot[i]; std::unique_lock<std::mutex> l(s.m); s.cv.wait(l, [&s] { return !s.queued && !s.running; }); s.job = std::move(f); s.queued = true; s.cv.notify_all(); }
    void wait(int i) { Slot &s = slot[i]; std::unique_lock<std::mutex> l(s.m); s.cv.wait(l, [&s] { return !s.queued && !s.running; }); }
    ~WalkerPool() { for (Slot &s : slot) if (s.th.joinable()) { { std::lock_guard<std::mutex> l(s.m); s.stop = true; } s.cv.notify_all(); s.th.join(); } }
};
WalkerPool &walker_pool() { static WalkerPool p; return p; }
// Walkers for the unit whose walk begins now: what its size asks for (walkers_wanted), one per CPU this process may use at most — its share of them when it is
// one of several ranks on the host (LOCAL_WORLD_SIZE: torch.distributed's launcher sets it), four at least.  The walks of a pipelined job overlap two or three
// at a time, so more walkers than CPUs are runnable for a millisecond or two; a CPU quota (cgroup cpu.max) bounds CPU time per period, not threads, and a job's
// walks use well under a third of it (bench.py: host_cpu_ms_per_step).  r03 first gave a walk half the CPUs (8 of 16): cfg3 jobs of 36.2 ms instead of 35.1.
inline int walkers_now(size_t n_pos) {
    const int want = walkers_wanted(n_pos);
    if (want <= 4 || getenv("AGX_WALK_SPLIT_WALKERS")) return want;
    static const int ranks = [] { const char *e = getenv("LOCAL_WORLD_SIZE"); const int n = e ? atoi(e) : 1; return n < 1 ? 1 : n; }();
    const int cpus = (int)usable_cpus() / ranks;
    return want <= cpus ? want : cpus < 4 ? 4 : cpus;
}

// units that exist in this process: when the last one is destroyed the output buffers parked for "the next unit" (agx_host.h: out_cache) go back to the C library — an embedder
// that never calls agx_pool_trim(-1) then keeps at most what it has itself given back since (up to 16 GB stayed resident until exit)
static std::atomic<int> g_units_alive{0};


namespace {

// One build at a time per device, on the GPU as well as in the launch order.  All builds of a device are queued on TWO streams, under a
// mutex that a host thread holds only while it enqueues its unit's kernel chain: `main` carries the node sweep and everything behind it
// (edge passes, walk preparation), `front` what comes before the sweep (zeroing, hit preparation, binning).  Units built from several
// host threads run their chains back to back — no host round trip in between — and the FRONT of build n+1 runs beside the BACK of build n:
// it starts when sweep n is done (an event) and sweep n+1 waits for it (another).  The node sweep itself never shares the device, so its
// HIP-event time is that of an exclusive GPU; the other sections are timed in exclusive builds (AGX_FLAG_TIME_SECTIONS serialises the two
// streams).
// Four streams per device serve all of its units: `up` carries the units' upload copies and nothing else, one unit after the other in the
// order they were queued (PCIe is one pipe: five uploads that share it all finish late; first in, first built, and its host walk runs
// beside the uploads of the rest); `front` and `main` carry the builds (see do_build); `down` the downloads.  Not a stream per unit: HIP
// maps its streams onto four hardware queues, and two streams that share one run their commands in the order they were queued — a
// build's first kernels sat 6 ms behind ANOTHER unit's upload copies, downloads 6-11 ms behind other units' kernels (profiles/r02_timeline_*.txt).
struct DeviceTurn { std::mutex m; hipStream_t main = nullptr, front = nullptr, up = nullptr, down = nullptr;
                    hipEvent_t sweep_done[2] = {nullptr, nullptr}, build_done[2] = {nullptr, nullptr};
                    unsigned long long n = 0; bool prev_exclusive = false; hipEvent_t prev_node = nullptr;      // n: builds queued so far; events alternate between two handles
                    std::mutex up_m, down_m, make_m;
                    void make() {       // (device current)
                        std::lock_guard<std::mutex> l(make_m);
                        if (main) return;
                        HIP_OK(hipStreamCreateWithFlags(&up, hipStreamNonBlocking)); HIP_OK(hipStreamCreateWithFlags(&front, hipStreamNonBlocking));
                        HIP_OK(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
                        for (auto &e : sweep_done) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                        for (auto &e : build_done) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                        HIP_OK(hipStreamCreateWithFlags(&main, hipStreamNonBlocking));
                    } };
DeviceTurn &turn_of(int device) { static DeviceTurn turns[64]; return turns[device & 63]; }

// AGX_TRACE_GAP=1: diagnostic for loops that rebuild long-lived units (see do_build)
static const bool g_trace_gap = getenv("AGX_TRACE_GAP") != nullptr;
// AGX_SCAN_LEGACY=1: the scans of a build as three launches each instead of one (decoupled look-back)
static const bool g_scan1 = getenv("AGX_SCAN_LEGACY") == nullptr;
// AGX_DEBUG_SYNC=1: synchronise after every launch group of a build and name it on stderr — a memory fault then points at its kernel
static const bool g_debug_sync = getenv("AGX_DEBUG_SYNC") != nullptr;
// AGX_TEST_SMALL_CAPS=1 (tests; read at every upload): every capacity starts absurdly small, so that every regrow path runs
#define g_tiny (getenv("AGX_TEST_SMALL_CAPS") != nullptr)
#define AGX_CHECKPOINT(name) do { if (g_debug_sync) { hipError_t e_ = hipStreamSynchronize(st); fprintf(stderr, "[agx debug] %s: %s\n", name, hipGetErrorString(e_)); } } while (0)

void join_dl_helper(agx_unit *u);
void drop_outputs(agx_unit *u);     // before a unit's inputs change: the helper that prepares the output buffers reads them
void start_helper(agx_unit *u);


// Where a streamed download cuts a unit of n_pos positions (r06): windows of about 4 M positions, 2 to AGX_DL_PIECES of them, at multiples of 64 ids (a word of the special-id bitmap,
// a tile of the side-id prefix).  None for units that one walker walks (nothing could begin earlier) or on request.  AGX_STREAM_PIECES=n forces n (tests: small units).
agx_cut_args stream_cuts(agx_u32 n_pos) {
    agx_cut_args C; memset(&C, 0, sizeof C);
    const char *force = getenv("AGX_STREAM_PIECES");
    if (getenv("AGX_NO_STREAM_DOWNLOAD") || n_pos < 4096) return C;
    size_t m = force ? (size_t)atoi(force) : n_pos < AGX_TWO_WALKERS_MIN ? 0 : n_pos / 4000000u;
    if (!force && m && m < 2) m = 2;
    if (m > AGX_DL_PIECES) m = AGX_DL_PIECES;
    if (m > n_pos / 1024u) m = n_pos / 1024u;
    for (size_t w = 0; w < m; w++) C.word[w] = (agx_u32)(((unsigned long long)n_pos * w / m) >> 6);
    C.word[m] = n_pos >> 6; C.n = (agx_u32)m;
    return C;
}


// ---- staging: the packed arrays a unit was handed, in the form and the memory the upload wants -------------------------------------
// Runs when the arrays are handed over (end of agx_unit_load_files, or agx_unit_stage after the last agx_unit_push_pairs; implied by an
// upload that finds nothing staged).  The read bases cross PCIe as 2-bit classes plus a list of the few bases that are not A, C, G or T
// (agx_pack_classes2): a quarter of the bytes of the largest array.  The read alignments are staged by stage_pairs() (agx_load.cpp) —
// or were written into the staged buffers by the fast loader while it parsed (u->pairs_staged).
// The arithmetic of every form is agx_forms.h, over plain arrays; what is here is the choice (u->choice, read once per entry: agx_unit.h), memory policy and the counts.
// The file-order wire records and read rows of a unit that will upload their tile-ordered forms (stage_tiled) are only ever read by the host — the gather into those forms, the
// cache file — so they live in ordinary memory: pinning a second copy of a unit's two largest arrays cost its load 0.2 ms per MB.  r05's forms (AGX_NO_TILED_UPLOAD) are uploaded
// from them and keep them pinned.
template <class B> inline void alloc_file_order(const agx_unit *u, B &buf, size_t count) { if (u->choice.tiled) buf.alloc_plain(count); else buf.alloc(count); }
// One of the six arrays of a unit's staged read alignments, for `bytes` of content: an element of slack each; the packed rows are asked for with their 16 bytes of slack.
void *alloc_pair_array(agx_unit *u, int which, size_t bytes) {
    switch (which) {
    case SA_HITS:  alloc_file_order(u, u->s_hits, bytes / sizeof(agx_whit) + 1); return u->s_hits.p;
    case SA_SIDES: u->s_sides.alloc(bytes / sizeof(agx_wside) + 1); return u->s_sides.p;
    case SA_RUNS:  u->s_runs.alloc(bytes / sizeof(agx_wrun) + 1); return u->s_runs.p;
    case SA_CODES: alloc_file_order(u, u->s_codes, bytes); return u->s_codes.p;
    case SA_JUMP:  u->s_jump.alloc(bytes / 4 + 1); return u->s_jump.p;
    default:       u->s_other.alloc(bytes / 8 + 1); return u->s_other.p;
    }
}
void alloc_pair_arrays(agx_unit *u) {      // all six, from the unit's counts (a staged-pairs file, a cache file)
    alloc_pair_array(u, SA_HITS, u->nh * sizeof(agx_whit)); alloc_pair_array(u, SA_SIDES, u->n_sides * sizeof(agx_wside)); alloc_pair_array(u, SA_JUMP, u->n_jump * 4);
    alloc_pair_array(u, SA_RUNS, u->n_runs * sizeof(agx_wrun)); alloc_pair_array(u, SA_CODES, u->n_codes + 16); alloc_pair_array(u, SA_OTHER, u->n_other * 8);
}
struct UnitSink : StageSink {
    agx_unit *u; explicit UnitSink(agx_unit *x) : u(x) {}
    void *take(int which, size_t bytes) override { return alloc_pair_array(u, which, bytes); }
};
void adopt_pairs(agx_unit *u, StagedPairs &S) {      // the staged read alignments' counts and the host-side row table
    u->nh = S.nh; u->n_runs = S.n_runs; u->n_sides = S.n_sides; u->n_jump = S.n_jump; u->n_codes = S.n_codes; u->n_other = S.n_other; u->stride = S.stride; u->maxlen = S.maxlen;
    u->pairs_in_file = S.n_pairs_in_file; u->sam_pairs = S.n_sam_pairs;
    u->row_off.swap(S.row_off); u->row_slot.swap(S.row_slot); u->n_rows = S.n_rows;
}
void stage_cm_layout(agx_unit *u, const agx_u8 *cm_cnt, size_t n_pos, const agx_cmseg *segs, size_t n_segs) {
    CmLayout L; build_cm_layout(cm_cnt, n_pos, segs, n_segs, L);
    u->n_cntruns = L.cnt_runs.size(); u->n_cntchunks = L.cnt_chunks.size(); u->n_segchunks = L.seg_chunks.size();
    u->s_cntruns.alloc(u->n_cntruns + 1); u->s_cntchunks.alloc(u->n_cntchunks + 1); u->s_segchunks.alloc(u->n_segchunks + 1);
    if (u->n_cntruns) memcpy(u->s_cntruns.p, L.cnt_runs.data(), u->n_cntruns * sizeof(agx_cntrun));
    if (u->n_cntchunks) memcpy(u->s_cntchunks.p, L.cnt_chunks.data(), u->n_cntchunks * sizeof(agx_chunk));
    if (u->n_segchunks) memcpy(u->s_segchunks.p, L.seg_chunks.data(), u->n_segchunks * sizeof(agx_chunk));
    build_seg_index(segs, u->n_seg0, n_pos, L.seg_index);
    u->n_segindex = L.seg_index.size(); u->s_segindex.alloc(u->n_segindex + 1); memcpy(u->s_segindex.p, L.seg_index.data(), u->n_segindex * 4);
}
// the unit sequence (+ appended positions) for the upload: 2 bits per base and the stretches of other bytes, or — a soft-masked sequence — the bytes themselves
void stage_reference(agx_unit *u, const char *ref, size_t n_pos, unsigned threads) {
    std::vector<agx_refx> others;
    u->s_ref.alloc((n_pos + 3) / 4 + 32);
    u->ref_packed = !u->choice.ref_raw && pack_reference(ref, n_pos, std::min(threads, 8u), u->s_ref.p, others);
    if (u->ref_packed) { u->n_refx = others.size(); u->s_refx.alloc(u->n_refx + 1); if (u->n_refx) memcpy(u->s_refx.p, others.data(), u->n_refx * sizeof(agx_refx)); return; }
    u->n_refx = 0; u->s_ref.alloc(n_pos + 16);
    const unsigned T = std::max(1u, std::min(threads, 8u));
    on_threads(T, [&](unsigned t) { const size_t lo = n_pos * t / T, hi = n_pos * (t + 1) / T; memcpy(u->s_ref.p + lo, ref + lo, hi - lo); });
}
// ---- the walk graph's way to the host ------------------------------------------------------------------------------------------------
// Every array of the walk graph that is downloaded is named ONCE, here: its pinned buffer, its source on the device, how many elements are copied — a function of the
// graph's four counts — and how many more the buffer holds behind them (the walk reads a little past some ends; the 64 bytes behind the meta bytes are zeroed).  The
// function shows them to a visitor, in the order a one-piece download copies them.  Buffers by estimate and exactly, the borrowed ones of a one-shot unit, the copy lists of
// both download forms, the release, download_bytes and what agx_unit_walk_graph hands out all work from it: a new array is one line here, plus the members.
struct GraphCounts { size_t n_pos, n_ids, n_special, n_ovf; };
enum { GA_BITS = 0, GA_RANK, GA_STR, GA_META, GA_XPOS, GA_NODE, GA_HOP, GA_OVF, GA_N };
template <class F> void graph_arrays(agx_unit *u, const GraphCounts &c, F f) {
    const size_t words = c.n_ids / 64 + 1, sides = c.n_ids - c.n_pos;
    f(GA_BITS, u->h_sp_bits, u->d_sp_bits, words, 1); f(GA_RANK, u->h_sp_rank, u->d_sp_rank, words, 1);      // the special ids: a bit per id, the records in front of every word
    f(GA_STR, u->h_a_str, u->d_a_str, c.n_ids, 1); f(GA_META, u->h_a_meta, u->d_a_meta, c.n_ids, 64);         // a base and a meta byte per id
    f(GA_XPOS, u->h_side_xpos, u->d_side_xpos, sides, 1);                                                    // the position of every side id
    f(GA_NODE, u->h_sp_node, u->d_sp_node, c.n_special, 1); f(GA_HOP, u->h_sp_hop, u->d_sp_hop, c.n_special, 2);      // the sparse record table
    f(GA_OVF, u->h_a_ovf, u->d_a_ovf, c.n_ovf, 1);                                                           // the edges that did not fit their records
}
// the one-shot download cuts its buffers from the dead staged blocks in this order: the largest arrays first, so that what does not fit any block is small
const int GRAPH_CUT_ORDER[GA_N] = {GA_NODE, GA_META, GA_STR, GA_HOP, GA_XPOS, GA_BITS, GA_RANK, GA_OVF};
inline GraphCounts graph_counts(const agx_unit *u) { return GraphCounts{u->V.n_pos, u->n_ids, u->n_special, u->n_ovf}; }
inline size_t graph_bytes(agx_unit *u, const GraphCounts &c) {      // what a download moves (stats.download_bytes, either form)
    size_t sum = 0; graph_arrays(u, c, [&](int, auto &h, auto &, size_t n, size_t) { sum += n * sizeof(*h.p); }); return sum;
}
// What a unit of n_pos positions is expected to download, where buffers are made before the build has counted:
// for the helper thread's pinned buffers (do_upload): walk ids ~ 1.05 x positions — an eighth of room —, special ids ~ 8 % of them; do_download re-sizes what is too small
inline GraphCounts helper_estimate(size_t n_pos) { const size_t ni = n_pos + n_pos / 8 + 4096; return GraphCounts{n_pos, ni, ni / 8 + 4096, 63}; }
// for the landing room of a one-shot unit (reserve_landing), which stays pinned as long as the staged unit does: a sixteenth of room, a tenth of the ids special
inline GraphCounts landing_estimate(size_t n_pos) { const size_t ni = n_pos + n_pos / 16 + 4096; return GraphCounts{n_pos, ni, ni / 10 + 4096, 0}; }

// The staged blocks that a one-shot unit's download may land in, in the order download_buffers cuts from them, the largest first: its inputs, dead once they are in HBM
// (`input`), and the landing block that reserve_landing sizes by what the inputs lack.
const int LANDING_ROOMS = 10;
template <class F> void landing_rooms(agx_unit *u, F f) {
    f(u->s_codes, true); f(u->s_hits, true); f(u->s_landing, false); f(u->s_codes_t, true); f(u->s_hits_t, true); f(u->s_runs, true); f(u->s_sides, true); f(u->s_other, true);
    f(u->s_wire, true); f(u->s_csides, true);      // (the compact wire forms; the tile-ordered records they stand for are ordinary memory then and count for nothing)
}

// A one-shot unit's download lands in the pinned memory of its staged inputs, which are dead once they are in HBM (do_download).  Since r03 those are packed
// (wire formats) and can be smaller than the walk graph: what is missing is pinned here, by estimate (landing_estimate), while the unit is staged — inside T_core
// mapping and registering it cost 1 ms per unit.  (`need` is a bound with slack of its own — 2 bytes per id, a record and a hop entry per special id, a quarter byte
// per id and 4 MB for the rest — not a sum over the arrays: it is left as it was, so that a unit pins what it pinned.)
void reserve_landing(agx_unit *u) {
    if (!(u->prm.flags & AGX_FLAG_ONE_SHOT)) { u->s_landing.release(); return; }
    const GraphCounts c = landing_estimate(u->V.n_pos); const size_t ni = c.n_ids, ns = c.n_special;
    const size_t need = 2 * (ni + 512) + ns * (sizeof(agx_walknode) + sizeof(agx_hop)) + ni / 4 + (4u << 20);
    size_t have = 0; landing_rooms(u, [&](auto &b, bool input) { if (input) have += b.block_bytes(); });
    // (a buffer must fit one block: count the blocks at 85 %)
    if (need > have * 85 / 100) u->s_landing.alloc(need - have * 85 / 100 + (ni + 512)); else u->s_landing.release();
}
// What the encoder of the read rows made (build_row_diffs), into the unit's pinned buffers: the rows cross as differences from now on.  For both stagers below.
void adopt_row_diffs(agx_unit *u, const RowDiffs &D, unsigned threads) {
    u->n_units = D.n_units; u->n_rowcnt = D.cnt.size(); u->n_blockoff = D.block_off.size(); u->n_blockfirst = D.block_first.size(); u->n_anchor = D.anchor_bits.size(); u->n_rows_explicit = D.n_explicit;
    u->s_units.alloc(u->n_units + 2); u->s_rowcnt.alloc(u->n_rowcnt); u->s_blockoff.alloc(u->n_blockoff); u->s_blockfirst.alloc(u->n_blockfirst); u->s_anchor.alloc(u->n_anchor);
    const unsigned T = std::max(1u, std::min(threads, 8u));
    on_threads(T, [&](unsigned t) { const size_t lo = u->n_units * t / T, hi = u->n_units * (t + 1) / T; if (hi > lo) memcpy(u->s_units.p + lo, D.units.data() + lo, (hi - lo) * 2); });
    memcpy(u->s_rowcnt.p, D.cnt.data(), u->n_rowcnt); memcpy(u->s_blockoff.p, D.block_off.data(), u->n_blockoff * 4); memcpy(u->s_blockfirst.p, D.block_first.data(), u->n_blockfirst * 4); memcpy(u->s_anchor.p, D.anchor_bits.data(), u->n_anchor * 4);
    u->rows_diffed = true;
}
void clear_row_diffs(agx_unit *u) { u->rows_diffed = false; u->n_units = u->n_rowcnt = u->n_blockoff = u->n_blockfirst = u->n_anchor = u->n_rows_explicit = 0; }
// The read rows for the upload as differences against the reference (agx_core.h; build_row_diffs in agx_load.cpp): AGX_ROW_DIFF=1 asks for it.  It is NOT the default:
// it takes 36-44 % off a unit's upload (66 -> 36 bytes per pair at 2x150) but no measured job is bound by its uploads — cfg3 36.4 against 36.5 ms, the 24-unit human
// shapes 50.0 against 49.4 ms (1/16) and 187 against 183 ms (1/4) per job — while making the form costs the loader 30-60 ns per row (T_unit + 0.1 s at cfg3).  For hosts
// whose ranks share a link or memory bandwidth.  Needs the packed reference.  The 2-bit rows stay where they are either way: the walk of a unit handed over staged reads
// k-mer tails out of them, and a one-shot unit's download lands in their memory.  This one: over the file-order rows (the tile-ordered forms have their own: stage_rows_tiled).
void stage_rows(agx_unit *u, unsigned threads) {
    if (!u->ref_packed || u->n_rows == 0 || u->nh == 0) return;
    const double t0 = now_ms();
    RowDiffs D;
    if (!build_row_diffs(u->s_hits.p, u->nh, u->s_sides.p, u->n_sides, u->s_runs.p, u->n_runs, u->s_codes.p, u->n_rows, u->stride, (const agx_u32 *)u->s_ref.p, u->V.n_pos ? u->V.n_pos : u->T.ref.size(), threads, D)) return;
    if (!row_diffs_gain(D, u->n_codes)) return;
    adopt_row_diffs(u, D, threads);
    if (getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] read rows against the reference: %.1f ms, %zu rows (%zu as they are), %.1f -> %.1f bytes per row\n", now_ms() - t0, (size_t)u->n_rows, u->n_rows_explicit,
                                          (double)u->n_codes / u->n_rows, (double)row_diffs_bytes(D) / u->n_rows);
}
// The hits in the order of the tile their first arrival falls in (agx_core.h "hits in tile order"; order_hits in agx_load.cpp): 4 bytes per hit + 4 per tile more to upload.
void stage_order(agx_unit *u, unsigned threads) {
    const double t0 = now_ms();
    const size_t n_pos = u->V.n_pos ? u->V.n_pos : u->T.ref.size(), n_tiles = (n_pos + AGX_TILE - 1) / AGX_TILE;
    u->lookback = agx_tile_lookback(u->maxlen, u->prm.k);
    u->s_perm.alloc(u->nh + 1); u->s_tfirst.alloc(n_tiles + 2); u->s_jump_at.alloc(u->n_jump + 1);
    order_hits(u->s_hits.p, u->nh, u->s_sides.p, u->s_runs.p, u->s_jump.p, u->n_jump, n_pos, threads, u->s_perm.p, u->s_tfirst.p, u->s_jump_at.p);
    if (getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] hits in tile order: %.1f ms (%zu hits, %zu tiles, window of %u tiles)\n", now_ms() - t0, u->nh, n_tiles, u->lookback);
}
// The staged read alignments in u->s_* as the content rules (agx_host.h: staged_pairs_rule, on what was read from a cache file or a staged-pairs file) and the tile-ordered
// gather look at them.
agx::StagedView staged_view(const agx_unit *u, unsigned long long n_rows, agx_u32 stride, agx_u32 maxlen, unsigned long long n_pos) {
    agx::StagedView V; V.hits = u->s_hits.p; V.nh = u->nh; V.sides = u->s_sides.p; V.n_sides = u->n_sides; V.runs = u->s_runs.p; V.n_runs = u->n_runs; V.jump = u->s_jump.p; V.n_jump = u->n_jump;
    V.other = u->s_other.p; V.n_other = u->n_other; V.n_rows = n_rows; V.stride = stride; V.maxlen = maxlen; V.n_pos = n_pos;
    return V;
}
// The hit and side records of the upload in their compact wire forms (agx_forms.h: HitPacker, plan_sides / fill_sides).  The blocks, escapes and extra words of the hits land in
// ONE pinned buffer of the size the records would have taken (s_wire): a unit pins what it pinned, and a one-shot unit's download finds the room it found.
void release_wire_hits(agx_unit *u) { u->hits_compact = false; u->n_cblocks = u->n_cesc = u->n_cext = 0; u->wire_esc = nullptr; u->wire_ext = nullptr; u->s_wire.release(); }
// what the packer made, noted in the unit; false: nothing gained (or the packer is off) — the unit sends its records
bool adopt_wire_hits(agx_unit *u, const HitPacker &P, const HitWire &W, double t0) {
    if (P.on && getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] compact hit records (with the forms they are made beside): %.1f ms, 16 -> %.2f bytes per hit, %.2f %% escaped, %.2f %% with an extra word%s\n", now_ms() - t0,
                                                  (double)W.bytes / u->nh, 100.0 * W.n_esc / u->nh, 100.0 * W.n_ext / u->nh, W.gain ? "" : ": not used");
    if (!W.gain) return false;
    u->wire_esc = W.esc; u->wire_ext = W.ext; u->n_cblocks = W.n_blocks; u->n_cesc = W.n_esc; u->n_cext = W.n_ext;
    return true;
}
// a unit that uploads r05's file-order forms: the blocks over s_hits
void stage_wire_hits(agx_unit *u, unsigned threads) {
    release_wire_hits(u);
    if (u->nh == 0) return;
    const double t0 = now_ms();
    HitPacker P(u->nh, u->maxlen, std::max(1u, std::min(threads, 16u)), u->choice.compact);
    if (P.on) { u->s_wire.alloc((u->nh + 1) * sizeof(agx_whit)); P.into(u->s_wire.p); P.pack_blocks(u->s_hits.p); }
    u->hits_compact = adopt_wire_hits(u, P, P.finish(), t0);
    if (!u->hits_compact) u->s_wire.release();
}
void stage_wire_sides(agx_unit *u) {
    u->sides_compact = false; u->n_csesc = 0; u->side_first = 0; u->wire_listed = nullptr;
    const size_t n = u->n_sides;
    const double t0 = now_ms();
    bool fine = u->choice.compact && n != 0;
    if (fine) {
        const SidePlan P = plan_sides(u->s_sides.p, n);
        u->side_first = P.first; fine = P.fine;
        if (fine) {
            u->s_csides.alloc(P.counts_bytes + (P.listed + 1) * sizeof(agx_cside_esc));
            agx_cside_esc *l = (agx_cside_esc *)(u->s_csides.p + P.counts_bytes);
            u->wire_listed = l; u->n_csesc = P.listed;
            fill_sides(u->s_sides.p, n, (agx_u16 *)u->s_csides.p, l);
        }
        if (getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] compact side records: %.1f ms, 12 -> %.2f bytes per side, %.2f %% listed%s\n", now_ms() - t0, (double)P.bytes / n,
                                              100.0 * P.listed / n, fine ? "" : ": not used (the run pool is not in side order, or nothing gained)");
    }
    if (!fine) { u->s_csides.release(); return; }
    u->sides_compact = true;
}

// r06: what the device is sent of the read alignments, in the order of the hits' first tiles (stage_order's permutation applied on the host; agx_forms.h: gather_tiled, with
// the hits packed inside the gather), and the windows the unit's first build sweeps as their rows land (do_upload / do_build).
void release_tiled(agx_unit *u) { u->tiled = false; u->n_other_t = 0; u->slot_row.clear(); u->n_win = 1; u->s_hits_t.release(); u->s_codes_t.release(); u->s_other_t.release(); }
void stage_tiled(agx_unit *u, unsigned threads) {
    const size_t nh = u->nh, s4 = u->stride / 4;
    const double t0 = now_ms();
    // (records that cross in their compact blocks are only ever read by the host: ordinary memory)
    if (u->choice.compact) u->s_hits_t.alloc_plain(nh + 1); else u->s_hits_t.alloc(nh + 1);
    u->s_codes_t.alloc(nh * s4 + 16); u->slot_row.resize(nh);
    const unsigned T = std::max(1u, std::min(threads, 16u));
    release_wire_hits(u);
    HitPacker packer(nh, u->maxlen, T, u->choice.compact);
    if (packer.on) { u->s_wire.alloc((nh + 1) * sizeof(agx_whit)); packer.into(u->s_wire.p); }
    const size_t n_pos = u->V.n_pos ? u->V.n_pos : u->T.ref.size(), n_tiles = (n_pos + AGX_TILE - 1) / AGX_TILE;
    const std::vector<unsigned long long> others = gather_tiled(staged_view(u, u->n_rows, u->stride, u->maxlen, n_pos), u->s_codes.p, u->s_perm.p, T, packer, u->s_hits_t.p, u->s_codes_t.p, u->slot_row.data());
    const size_t no = others.size();
    u->s_other_t.alloc(no + 1); u->n_other_t = no;
    if (no) memcpy(u->s_other_t.p, others.data(), no * 8);
    u->tiled = true;
    u->hits_compact = adopt_wire_hits(u, packer, packer.finish(), t0);
    if (u->choice.compact && !u->hits_compact) {      // nothing gained: the records into the pinned buffer that the blocks would have filled
        u->s_wire.alloc((nh + 1) * sizeof(agx_whit));
        on_threads(T, [&](unsigned t) { const size_t lo = nh * t / T, hi = nh * (t + 1) / T; if (hi > lo) memcpy(u->s_wire.p + lo * sizeof(agx_whit), u->s_hits_t.p + lo, (hi - lo) * sizeof(agx_whit)); });
    }
    u->n_win = window_cuts(n_pos, n_tiles, u->choice.windows, u->win_tile);
    if (getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] tile-ordered upload forms: %.1f ms (%zu hits, %zu listed bases, %u windows)\n", now_ms() - t0, nh, no, u->n_win);
}

// r06: the read rows of the tile-ordered forms as their differences from the reference (agx_core.h "read rows relative to the reference"): row i is hit i's left mate, so every
// row's anchor is its own hit — no anchor search, no order condition — and the encoder and the device's decoder are r04's (build_row_diffs with rows_are_hits; agx_k_expand_rows
// over anchor bits that are all ones).  The stream of differences is in row order = tile order: a window's rows are one piece of it (do_upload), expanded when it has landed.
// WHEN ("by a rule in code ... or delete the lines"): measured on the round's last tree (profiles/r06_l_*), the rule is NEVER by itself.  The form takes 35-38 %
// off a unit's upload (cfg3 1.13 -> 0.74 GB per job, rank 0 of 8 of configs[4] 3.76 -> 2.34 GB) and costs the unit's first build the slower expansion (agx_k_expand_rows: a
// lane per row decodes its row into LDS; ~10 ms for chr1's 33 M rows of 150 bases against 1 ms of agx_k_expand_codes) and the loader 30-60 ns per row (t_unit_s 0.42 -> 0.62 s at
// cfg3).  Since the windows, a unit's kernels run beside its upload and the two are about as long: with a third of the bytes gone the kernels bind, and they are the longer for
// it — chr1 in the emulated rank is built at 66.9 ms instead of 61.9, the rank done at 132.6 instead of 128.7 ms; cfg3's builds end 0.6 ms later each.  It stays what it was
// in r04/r05: an option for hosts whose link is scarcer than this one's (AGX_ROW_DIFF=1; =0 or unset: the 2-bit rows), parity-tested both ways in both upload forms.
// Where the form does not apply (a raw reference, a stride beyond the codec's) or gains nothing, the unit's 2-bit rows cross tile-ordered.
void stage_rows_tiled(agx_unit *u, unsigned threads) {
    if (!u->ref_packed || u->stride > AGX_ROW_MAXSTRIDE) return;
    const size_t n_pos = u->V.n_pos ? u->V.n_pos : u->T.ref.size();
    const double t0 = now_ms();
    RowDiffs D;
    if (!build_row_diffs(u->s_hits_t.p, u->nh, u->s_sides.p, u->n_sides, u->s_runs.p, u->n_runs, u->s_codes_t.p, u->nh, u->stride, (const agx_u32 *)u->s_ref.p, n_pos, threads, D, true)) return;
    if (!row_diffs_gain(D, u->nh * (u->stride / 4))) return;
    adopt_row_diffs(u, D, threads);
    if (getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] tile-ordered rows against the reference: %.1f ms, %zu rows (%zu as they are), %.1f -> %.1f bytes per row\n", now_ms() - t0, u->nh, u->n_rows_explicit,
                                          (double)(u->stride / 4), (double)row_diffs_bytes(D) / u->nh);
}

// The tail of staging, from the text (stage_inputs) and from the cache file (load_cache) alike, once the unit's view and its file-order arrays are there: the upload forms
// of the rows and the hits by the unit's choice (DESIGN.md "Upload forms" has this as a table), the landing room of a one-shot download; the unit is staged and nothing of an
// earlier upload counts any more.
void finish_staging(agx_unit *u, unsigned threads_rows, unsigned threads) {
    clear_row_diffs(u);
    if (u->choice.tiled && u->nh != 0 && u->n_rows != 0) {      // the tile-ordered forms, the hits packed inside the gather
        stage_order(u, threads);
        stage_tiled(u, threads);
        if (u->choice.row_diff) stage_rows_tiled(u, threads);
    } else {                                                    // the file-order forms, the hits packed over s_hits
        release_tiled(u);
        if (u->choice.row_diff) stage_rows(u, threads_rows);
        stage_order(u, threads);
        stage_wire_hits(u, threads);
    }
    stage_wire_sides(u);
    u->V.slot_row = u->tiled ? u->slot_row.data() : nullptr;
    reserve_landing(u);
    u->staged = true; u->consumed = false; u->uploaded = false; u->built = false; u->downloaded = false;
}

void stage_inputs(agx_unit *u) {
    u->choice = upload_choice();
    if (!u->have_ref || !u->have_threads) throw Error{E_ARG, "reference and contig threads must be set before upload"};
    // A one-shot unit's download lands in its staged buffers.  The general loader's pairs can be staged again from P; the fast loader wrote the hits, runs and
    // codes straight into those buffers and kept nothing else: after the download there is nothing to stage from, and clearing `consumed` would send the walk
    // graph's bytes to the device as wire records.
    if (u->consumed && u->pairs_staged) throw Error{E_ARG, "one-shot unit: its staged read alignments were overwritten by the download; load the unit again"};
    const double t0 = now_ms();
    HIP_OK(hipSetDevice(u->prm.device));            // (registering host memory needs a current device)
    u->cache_map.reset(); u->reads_map.reset();
    const size_t n_pos = u->T.ref.size();
    if (n_pos == 0 || n_pos >= 0xFFFFFF00ull) throw Error{E_ARG, "unit sequence is empty or too long"};
    if (u->T.cm_cnt.size() != n_pos) throw Error{E_ARG, "conti-mer chains were not built"};
    { size_t el = 0; for (const agx_cmseg &g : u->T.segs) el += g.len; if (el != u->T.n_cm) throw Error{E_ARG, "conti-mer runs were not built"}; }
    u->n_seg0 = u->T.n_seg0; u->n_cm = u->T.n_cm;
    u->n_segs = u->T.segs.size(); u->s_segs.alloc(u->n_segs + 1);
    if (u->n_segs) memcpy(u->s_segs.p, u->T.segs.data(), u->n_segs * sizeof(agx_cmseg));
    std::vector<agx_u32> ce(u->T.chain_end_pos); std::sort(ce.begin(), ce.end()); ce.erase(std::unique(ce.begin(), ce.end()), ce.end());      // positions where a conti-mer chain
    u->n_chain_end = (agx_u32)ce.size(); u->s_chain_end.alloc(ce.size() + 1);                                                                 // ends: their main walk ids are special
    if (!ce.empty()) memcpy(u->s_chain_end.p, ce.data(), ce.size() * 4);
    const unsigned threads = loader_threads(u->P.bases.size() + n_pos + u->nh * 64);
    stage_reference(u, u->T.ref.data(), n_pos, threads);
    stage_cm_layout(u, u->T.cm_cnt.data(), n_pos, u->T.segs.data(), u->n_segs);
    if (!u->pairs_staged) {
        UnitSink sink(u); StagedPairs S;
        u->n_slots = u->P.n_slots;
        stage_pairs(u->P, u->prm.k, threads, sink, S);
        adopt_pairs(u, S);
    }
    UnitView V = view_of(u->T, u->P);
    if (u->pairs_staged && u->pairs_file.fv) {      // staged pairs from their file: no read bases but the 2-bit rows
        const agx::PairsFile &F = u->pairs_file;
        V.bases = nullptr; V.row_off = nullptr; V.stride = u->stride; V.codes2 = (const agx_u8 *)F.sec(pairsfile::S_CODES);
        V.other_idx = (const unsigned long long *)F.sec(pairsfile::S_OTHER); V.other_byte = (const agx_u8 *)F.sec(pairsfile::S_OTHERB); V.n_other = (size_t)F.H.n_other;
    } else if (u->pairs_staged) { V.bases = u->reads_keep ? u->reads_keep->fv.p : nullptr; V.stride = u->stride; V.row_off = u->row_off.data(); }
    u->V = V; u->n_chain_str = u->T.chain_str.size();
    finish_staging(u, threads, threads);
    u->stats.ms_stage = now_ms() - t0;
}

// ---- unit cache file ----------------------------------------------------------------------------------------------------------------
// tmp/_agx_unit.<u>.bin: a unit's STAGED form, written once (AlignGraph_amd does it when it distributes the alignments, AG:3545-3579;
// agx_unit_cache_build) so that a unit loop that finds it neither reads nor parses text: the arrays the upload wants are read straight into
// pinned memory, what only the host walk looks at (conti-mer counts, chain suffixes, read bases for the k-mer tails of written records) is
// mapped and paged in where it is touched.  Valid for one BATCH size, one k and for exactly the five text files it was made from (size and
// modification time of each are in the header): anything else and the loader falls back to the text.
namespace cache {
using namespace agx::cachefile;      // the header and the section numbers (agx_host.h)
void stamps(const std::string &d, int unit, unsigned long long st[6][2]) {
    const std::string s = std::to_string(unit);
    const std::string f[6] = {d + "/_genome." + s + ".fa", d + "/_contigs.fa", d + "/_contigs_genome." + s + ".psl", d + "/_reads.fa", d + "/_reads_genome." + s + ".bowtie", pairsfile::path_of(d, unit)};
    for (int i = 0; i < 6; i++) { struct stat sb; if (stat(f[i].c_str(), &sb) != 0) { st[i][0] = st[i][1] = ~0ull; continue; }
        st[i][0] = (unsigned long long)sb.st_size; st[i][1] = (unsigned long long)sb.st_mtim.tv_sec * 1000000000ull + (unsigned long long)sb.st_mtim.tv_nsec; }
}
std::string path_of(const std::string &d, int unit) { return d + "/_agx_unit." + std::to_string(unit) + ".bin"; }
}  // namespace cache

// Large arrays between memory and a file or a mapping, in pieces of 32 MB on a few threads.  A piece names its memory and the other side's offset; step(memory, offset, bytes)
// moves up to that many bytes and returns how many it did (memcpy, pread, pwrite; <= 0: failed).  false: some piece failed.
struct Piece { char *mem; unsigned long long off, len; };
void cut_pieces(std::vector<Piece> &pieces, const void *mem, unsigned long long off, unsigned long long len) {
    for (unsigned long long a = 0; a < len; a += 32ull << 20) pieces.push_back(Piece{(char *)mem + a, off + a, std::min<unsigned long long>(32ull << 20, len - a)});
}
template <class Step> bool move_pieces(const std::vector<Piece> &pieces, unsigned threads, Step step) {
    std::vector<int> bad(threads, 0);
    on_threads(threads, [&](unsigned t) {
        for (size_t i = t; i < pieces.size(); i += threads)
            for (size_t done = 0; done < pieces[i].len;) { const ssize_t r = step(pieces[i].mem + done, pieces[i].off + done, (size_t)(pieces[i].len - done)); if (r <= 0) { bad[t] = 1; return; } done += (size_t)r; }
    });
    return std::find(bad.begin(), bad.end(), 1) == bad.end();
}

void save_cache(agx_unit *u, const std::string &dir, int unit) {
    using namespace cache;
    if (!u->staged || u->cache_map.p) throw Error{E_ARG, "nothing staged from text"};
    Header H; memset(&H, 0, sizeof H); memcpy(H.magic, MAGIC, 8); H.version = 2; H.batch = u->prm.batch;
    stamps(dir, unit, H.stamp);
    const bool from_codes = u->pairs_staged && u->pairs_file.fv, in_reads = u->pairs_staged && !from_codes;
    H.n_pos = u->V.n_pos; H.n_ref = u->V.n_ref; H.nh = u->nh; H.n_runs = u->n_runs; H.n_cm = u->n_cm; H.n_segs = u->n_segs; H.n_seg0 = u->n_seg0; H.n_rows = u->n_rows;
    H.n_chain_end = u->n_chain_end; H.n_codes = u->n_codes; H.pairs_in_file = u->pairs_in_file; H.sam_pairs = u->sam_pairs; H.stride = u->stride; H.maxlen = u->maxlen; H.n_slots = u->n_slots; H.k = u->prm.k;
    H.rows_in_reads = from_codes ? 2u : in_reads ? 1u : 0u; H.sizes[0] = sizeof(agx_whit); H.sizes[1] = sizeof(agx_wrun); H.sizes[2] = sizeof(agx_cmseg); H.sizes[3] = sizeof(Header); H.sizes[4] = sizeof(agx_wside);
    H.slot_stride = u->V.stride; H.n_sides = u->n_sides; H.n_jump = u->n_jump;
    const void *ptr[S_N] = {u->s_hits.p, u->s_runs.p, u->s_codes.p, u->s_segs.p, u->s_chain_end.p, from_codes ? nullptr : in_reads ? (const void *)u->row_off.data() : (const void *)u->row_slot.data(), u->V.ref, u->V.cm_cnt,
                            u->V.chain_str, u->V.initial, (in_reads || from_codes) ? nullptr : u->V.bases, u->s_other.p, u->s_sides.p, u->s_jump.p, from_codes ? (const void *)u->V.other_byte : nullptr};
    const unsigned long long len[S_N] = {u->nh * sizeof(agx_whit), u->n_runs * sizeof(agx_wrun), u->n_codes, u->n_segs * sizeof(agx_cmseg), (unsigned long long)u->n_chain_end * 4, from_codes ? 0ull : (unsigned long long)u->n_rows * (in_reads ? 8 : 4),
                                         u->V.n_pos, u->V.n_pos, u->T.chain_str.size(), u->V.n_initial, (in_reads || from_codes) ? 0ull : (unsigned long long)u->n_slots * u->V.stride, (unsigned long long)u->n_other * 8,
                                         u->n_sides * sizeof(agx_wside), (unsigned long long)u->n_jump * 4, from_codes ? (unsigned long long)u->n_other : 0ull};
    unsigned long long at = (sizeof(Header) + 4095) & ~4095ull;
    for (int i = 0; i < S_N; i++) { H.off[i] = at; H.len[i] = len[i]; at = (at + len[i] + 4095) & ~4095ull; }
    const std::string path = path_of(dir, unit), part = path + ".part";
    const int fd = open(part.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) throw Error{E_IO, "CANNOT OPEN FILE! (" + part + ")"};
    bool ok = ftruncate(fd, (off_t)at) == 0 && pwrite(fd, &H, sizeof H, 0) == (ssize_t)sizeof H;
    if (ok) {      // the sections, large pieces on a few threads
        std::vector<Piece> pieces;
        for (int i = 0; i < S_N; i++) cut_pieces(pieces, ptr[i], H.off[i], len[i]);
        ok = move_pieces(pieces, (unsigned)std::min<size_t>(8, pieces.size() ? pieces.size() : 1), [&](char *mem, unsigned long long off, size_t n) { return pwrite(fd, mem, n, (off_t)off); });
    }
    ok = (close(fd) == 0) && ok;
    if (!ok || rename(part.c_str(), path.c_str()) != 0) { (void)remove(part.c_str()); throw Error{E_IO, "cannot write " + path}; }
}

// A unit's read alignments out of tmp/_agx_pairs.<u>.bin (agx_host.h: pairsfile): the arrays into the pinned upload buffers, checked like a cache file's; the mapped file stays
// with the unit (the walk takes the k-mer tails of written records from its 2-bit rows).
void load_staged_pairs(agx_unit *u, agx::PairsFile &F) {
    using namespace pairsfile;
    const Header &H = F.H;
    if (pairs_unit_rule(H, u->prm.k, u->prm.batch)) throw Error{E_ARG, "tmp/_agx_pairs: staged for another k or another BATCH than this unit's"};
    u->nh = H.nh; u->n_runs = H.n_runs; u->n_sides = H.n_sides; u->n_jump = H.n_jump; u->n_codes = H.n_codes; u->n_other = H.n_other; u->stride = H.stride; u->maxlen = H.maxlen; u->n_rows = H.n_rows;
    u->pairs_in_file = H.pairs_in_file; u->sam_pairs = H.sam_pairs; u->n_slots = 0; u->row_off.clear(); u->row_slot.clear(); u->reads_keep.reset(); u->reads_map.reset();
    alloc_pair_arrays(u);
    std::vector<Piece> pieces;
    auto cut = [&](void *dst, int sec) { cut_pieces(pieces, dst, H.off[sec], H.len[sec]); };
    cut(u->s_hits.p, S_HITS); cut(u->s_sides.p, S_SIDES); cut(u->s_jump.p, S_JUMP); cut(u->s_runs.p, S_RUNS); cut(u->s_codes.p, S_CODES); cut(u->s_other.p, S_OTHER);
    const unsigned threads = (unsigned)std::min<size_t>(std::min<unsigned>(8u, std::max(1u, usable_cpus())), pieces.size() ? pieces.size() : 1);
    move_pieces(pieces, threads, [&](char *mem, unsigned long long off, size_t n) { memcpy(mem, F.fv->p + off, n); return (ssize_t)n; });
    const char *rule = staged_pairs_rule(staged_view(u, H.n_rows, H.stride, H.maxlen, 0), threads);      // (the unit's positions are not known yet: agx_unit_load_files_shared)
    if (!rule) rule = other_ascending_rule(u->s_other.p, u->n_other);      // (the walk bisects the list)
    if (rule) throw Error{E_FORMAT, std::string("tmp/_agx_pairs: the staged arrays are inconsistent (") + rule + ")"};
    u->pairs_staged = true; u->pairs_file = std::move(F);
}

// true: the unit is staged from the cache file.  false: no usable cache (missing, another batch size, older than its sources, damaged).
bool load_cache(agx_unit *u, const std::string &dir, int unit) {
    using namespace cache;
    if (getenv("AGX_NO_CACHE")) return false;
    const std::string path = path_of(dir, unit);
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
    Header H; struct stat sb;
    if (fstat(fd, &sb) != 0 || (size_t)sb.st_size < sizeof H || pread(fd, &H, sizeof H, 0) != (ssize_t)sizeof H) return false;
    unsigned long long st[6][2]; stamps(dir, unit, st);
    if (cache_header_rule(H, (unsigned long long)sb.st_size, u->prm.batch, u->prm.k) || memcmp(st, H.stamp, sizeof st) != 0) return false;
    const bool in_reads = H.rows_in_reads == 1, from_codes = H.rows_in_reads == 2;
    HIP_OK(hipSetDevice(u->prm.device));
    const double t0 = now_ms();
    std::unique_ptr<FileView> reads_map;
    if (in_reads) { try { reads_map.reset(new FileView(dir + "/_reads.fa")); } catch (const Error &) { return false; } if (reads_map->n != st[3][0]) return false; }
    void *m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) return false;
    drop_outputs(u);
    u->T = Threads(); u->P = Pairs(); u->cache_map.reset(); u->cache_map.p = m; u->cache_map.n = (size_t)sb.st_size; u->reads_keep.reset(); u->reads_map.reset(); u->pairs_file = agx::PairsFile();
    const char *base = (const char *)m;
    u->nh = H.nh; u->n_runs = H.n_runs; u->n_sides = H.n_sides; u->n_jump = H.n_jump; u->n_cm = H.n_cm; u->n_segs = H.n_segs; u->n_seg0 = (agx_u32)H.n_seg0; u->n_chain_end = (agx_u32)H.n_chain_end; u->n_codes = H.n_codes; u->n_other = H.len[S_OTHER] / 8;
    u->pairs_in_file = H.pairs_in_file; u->sam_pairs = H.sam_pairs; u->stride = H.stride; u->maxlen = H.maxlen; u->n_slots = H.n_slots; u->n_rows = (agx_u32)H.n_rows;
    alloc_pair_arrays(u); u->s_segs.alloc(u->n_segs + 1); u->s_chain_end.alloc((size_t)u->n_chain_end + 1);
    // the staged arrays: read into the pinned buffers, a few threads, large pieces
    std::vector<Piece> pieces;
    auto cut = [&](void *dst, int sec) { cut_pieces(pieces, dst, H.off[sec], H.len[sec]); };
    cut(u->s_hits.p, S_HITS); cut(u->s_sides.p, S_SIDES); cut(u->s_jump.p, S_JUMP); cut(u->s_runs.p, S_RUNS); cut(u->s_codes.p, S_CODES); cut(u->s_other.p, S_OTHER); cut(u->s_segs.p, S_SEGS); cut(u->s_chain_end.p, S_CHAIN_END);
    const unsigned threads = (unsigned)std::min<size_t>(std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency())), pieces.size() ? pieces.size() : 1);
    bool fine = move_pieces(pieces, threads, [&](char *mem, unsigned long long off, size_t n) { return pread(fd, mem, n, (off_t)off); });
    // what the device and the walk index with must be in range: a file whose lengths are intact but whose content is not is a reason to parse the text again, not to read out of bounds
    if (fine) {
        agx::CacheView C; C.segs = u->s_segs.p; C.n_segs = u->n_segs; C.cm_cnt = (const agx_u8 *)(base + H.off[S_CM_CNT]); C.chain_end = u->s_chain_end.p; C.n_chain_end = u->n_chain_end;
        C.rows = base + H.off[S_ROWS]; C.n_pos = H.n_pos; C.n_cm = H.n_cm; C.n_rows = H.n_rows; C.chain_str_len = H.len[S_CHAIN_STR]; C.reads_size = in_reads ? reads_map->n : 0;
        C.maxlen = H.maxlen; C.n_slots = H.n_slots; C.rows_in_reads = H.rows_in_reads;
        fine = !staged_pairs_rule(staged_view(u, H.n_rows, H.stride, H.maxlen, H.n_pos), threads) && !cache_content_rule(C, threads) && !(from_codes && other_ascending_rule(u->s_other.p, u->n_other));
    }
    if (!fine) { u->cache_map.reset(); return false; }
    const double tv = now_ms();
    stage_reference(u, base + H.off[S_REF], H.n_pos, threads);
    const double tr = now_ms();
    stage_cm_layout(u, (const agx_u8 *)(base + H.off[S_CM_CNT]), H.n_pos, u->s_segs.p, u->n_segs);
    if (getenv("AGX_LOAD_TIMING")) fprintf(stderr, "[agx load] cache: buffers + read + checks %.1f ms, reference %.1f ms, conti-mer layout %.1f ms\n", tv - t0, tr - tv, now_ms() - tr);
    UnitView V; V.ref = base + H.off[S_REF]; V.n_pos = H.n_pos; V.n_ref = (agx_u32)H.n_ref; V.cm_cnt = (const agx_u8 *)(base + H.off[S_CM_CNT]); V.chain_str = base + H.off[S_CHAIN_STR];
    V.hop = nullptr; V.segs = (const agx_cmseg *)(base + H.off[S_SEGS]); V.n_seg0 = (agx_u32)H.n_seg0; V.stride = (in_reads || from_codes) ? H.stride : H.slot_stride; V.initial = base + H.off[S_INITIAL]; V.n_initial = H.len[S_INITIAL];
    u->row_off.clear(); u->row_slot.clear();
    if (from_codes) { V.bases = nullptr; V.codes2 = (const agx_u8 *)(base + H.off[S_CODES]); V.other_idx = (const unsigned long long *)(base + H.off[S_OTHER]); V.other_byte = (const agx_u8 *)(base + H.off[S_OTHERB]); V.n_other = u->n_other; }
    else if (in_reads) { u->reads_map = std::move(reads_map); V.bases = u->reads_map->p; V.row_off = (const uint64_t *)(base + H.off[S_ROWS]); }
    else { V.bases = base + H.off[S_BASES]; u->row_slot.assign((const agx_u32 *)(base + H.off[S_ROWS]), (const agx_u32 *)(base + H.off[S_ROWS]) + H.n_rows); }
    u->V = V; u->n_chain_str = (size_t)H.len[S_CHAIN_STR]; u->pairs_staged = false;
    finish_staging(u, std::max(threads, std::min(8u, usable_cpus())), std::max(threads, std::min(16u, usable_cpus())));
    u->have_ref = u->have_threads = true;
    u->stats.ms_stage = now_ms() - t0; u->stats.ms_parse = 0; u->stats.ms_thread = 0; u->stats.from_cache = 1;
    return true;
}

// ---- capacities ---------------------------------------------------------------------------------------------------------------------
// First guesses, made so that a unit's first build is normally its only one (every capacity is still checked on the device and grown
// from the device-side counters if it proves too small: tests force that with AGX_TEST_SMALL_CAPS).
agx_u32 spill_min(const agx_unit *u) { const size_t n_pos = u->V.n_pos; return (agx_u32)std::min<size_t>(g_tiny ? 64 : n_pos / 8 + 65536, 0x10000000u); }

// Slices of the node pool, one per region, and the spill area behind them.  Without a measurement every region gets the same share of
// `main_cap` ids; after a build in which the pool ran out, `demand` holds what every region asked for (the counters keep counting) and the
// slices are cut to that plus slack.  Returns the ids the layout needs; applies it (queues the copy on `st`, and adds its bytes to `sent`) if they fit.
unsigned long long layout_regions(agx_unit *u, const agx_u32 *demand, agx_u32 main_cap, bool apply, hipStream_t st, size_t *sent = nullptr) {
    const agx_u32 R = u->n_regions;
    u->s_region_off.alloc((size_t)R + 1);
    agx_u32 *off = u->s_region_off.p;
    unsigned long long at = 0;
    for (agx_u32 r = 0; r < R; r++) {
        off[r] = (agx_u32)std::min<unsigned long long>(at, 0xFFFFFFFFull);
        at += demand ? (unsigned long long)demand[r] + demand[r] / 8 + 64 : main_cap / R;
    }
    const unsigned long long need = at + spill_min(u);
    if (!apply || need > u->pool_cap) return need;
    off[R] = (agx_u32)at; u->spill_lo = (agx_u32)at;
    HIP_OK(hipMemcpyAsync(u->d_region_off.p, off, ((size_t)R + 1) * 4, hipMemcpyHostToDevice, st));
    if (sent) *sent += ((size_t)R + 1) * 4;
    return need;
}

// ---- a unit's device buffers ---------------------------------------------------------------------------------------------------------
// Every buffer a unit takes with its block is named ONCE, with its element count, in one of five groups: the groups are what regrows separately.  A group is a function
// that shows its buffers, in the order they lie in the block, to a Take.  On a const unit that only adds up their bytes (plan_capacities: what the block must hold,
// whatever the views hold now); with an arena, on a unit that is uploaded or regrown, it also takes them from it (the arena keeps what a regrown group leaves behind until
// the unit is released) and notes in the unit what the group was sized by.  A new buffer is one line in its group, plus the member.
struct Take {
    DevArena *arena = nullptr; size_t bytes = 0;
    template <class B> void operator()(B &b, size_t count) {
        bytes += (count * sizeof(*b.p) + 255) & ~(size_t)255;      // (DevArena::take's alignment)
        if constexpr (!std::is_const_v<B>) if (arena) { b.release(); b.alloc(*arena, count); }
    }
    template <class M> void note(M &member, size_t v) { if constexpr (!std::is_const_v<M>) if (arena) member = (M)v; }
};
inline size_t codes_bytes(const agx_unit *u) { return u->tiled ? u->nh * (u->stride / 4) : u->n_codes; }      // packed read rows as they are uploaded (tile-ordered: one row per hit)
inline size_t others_up(const agx_unit *u) { return u->tiled ? u->n_other_t : u->n_other; }
inline agx_u32 tiles_of(const agx_unit *u) { return (agx_u32)((u->V.n_pos + AGX_TILE - 1) / AGX_TILE); }
inline agx_u32 regions_of(const agx_unit *u) { return (tiles_of(u) + AGX_REGION_TILES - 1) / AGX_REGION_TILES; }
inline agx_u32 words_of(const agx_unit *u, agx_u32 pool_cap) { return (agx_u32)((u->V.n_pos + pool_cap) / 64 + 1); }      // 64 walk ids per word of the sparse table's bit vector
inline size_t scan_desc_of(const agx_unit *u, agx_u32 pool_cap) { return (std::max<size_t>(tiles_of(u), words_of(u, pool_cap)) + 1) / 4096 + 2; }

// the node pool and what is indexed by walk id (side variants <= nodes <= pool_cap)
template <class U> void pool_bufs(U *u, agx_u32 cap, Take &t) {
    const size_t n_pos = u->V.n_pos, ids_cap = n_pos + cap, n_words = words_of(u, cap);
    t.note(u->pool_cap, cap); t.note(u->n_words, n_words); t.note(u->scan_desc_n, scan_desc_of(u, cap));
    const size_t kcap = (size_t)cap + AGX_SLOW_V;      // slack: the edge pass reads whole AGX_SLOW_V-row batches of keys (agx_edge_slow_ctx)
    // First what the host walk may still ask the device for after the download (agx_walk_record through fetch_records: the records of ids outside the sparse table): the walk id
    // and node of every id, and four node arrays — 40 bytes per node slot + 4 per id, a quarter of the unit's block.  They lie at the FRONT of the block so that everything
    // behind them can go back to the device when the download is done (agx_unit_trim), not when the walk is (r05: on the whole-human job a unit's walk takes longer than its
    // upload and build, and the units waiting for room on the device were waiting for walks).
    t(u->d_aid_of, (size_t)cap + 1); t(u->d_a_nid, ids_cap + 1); t(u->d_off0, kcap); t(u->d_sref, cap); t(u->d_next, (size_t)cap * AGX_MAXE); t(u->d_fetch, 65536);
    t.note(u->keep_end, t.arena ? t.arena->first_block_at() : 0);      // (do_trim; ~0: this pool is a regrown one in a later block)
    t(u->d_cid, kcap); t(u->d_coff, kcap); t(u->d_cid0, kcap); t(u->d_coff0, kcap); t(u->d_base, cap); t(u->d_flags, cap);
    if (u->prm.flags & AGX_FLAG_KEEP_COUNTS) t(u->d_counts, (size_t)cap * 6);
    if (u->prm.flags & AGX_FLAG_EDGE_SUPPORT) t(u->d_e_cnt, (size_t)cap * AGX_MAXE);
    t(u->d_a_str, ids_cap + 1); t(u->d_a_meta, ids_cap + 16); t(u->d_a_mark, ids_cap + 2); t(u->d_side_xpos, (size_t)cap + 1);
    t(u->d_sp_bits, n_words + 1); t(u->d_sp_cnt, n_words + 1); t(u->d_sp_rank, n_words + 2);
    const size_t nb = (std::max<size_t>(n_pos, n_words) + 1 + 1023) / 1024;
    t(u->d_scan_tmp, 2 * (nb + 1) + 2 * ((nb + 1023) / 1024 + 1) + 16); t(u->d_scan_desc, 3 * scan_desc_of(u, cap));      // (descriptors of the three one-launch scans)
}
// what never regrows: the inputs in their upload forms, the arrays derived from them per position, tile and hit, scratch, counters
template <class U> void fixed_bufs(U *u, Take &t) {
    const size_t n_pos = u->V.n_pos, nh = u->nh, n_tiles = tiles_of(u), n_regions = regions_of(u);
    t(u->d_cm_start, n_pos + 2); t(u->d_cm, u->n_cm + 1); t(u->d_ref, n_pos + 16); t(u->d_cm_head, n_pos + 1);
    t(u->d_segs, u->n_segs + 1); t(u->d_cntruns, u->n_cntruns + 1); t(u->d_cntchunks, u->n_cntchunks + 1); t(u->d_segchunks, u->n_segchunks + 1); t(u->d_segindex, u->n_segindex + 1);
    t(u->d_runs, u->n_runs + 1); t(u->d_vcodes, codes_bytes(u) * 4 + 16); t(u->d_other, others_up(u) + 1);
    if (u->rows_diffed) { t(u->d_units, u->n_units + 2); t(u->d_rowcnt, u->n_rowcnt); t(u->d_blockoff, u->n_blockoff); t(u->d_blockfirst, u->n_blockfirst); t(u->d_anchor, u->n_anchor); }
    else t(u->d_codes, codes_bytes(u) + 16);
    if (u->hits_compact) { t(u->d_chits, u->n_cblocks + 1); t(u->d_cesc, u->n_cesc + 1); t(u->d_cext, u->n_cext + 1); }
    if (u->sides_compact) { t(u->d_csides, u->n_sides + 1); t(u->d_csesc, u->n_csesc + 1); t(u->d_cside_scan, agx_side_scan_words(u->n_sides)); }
    t(u->d_whits, nh + 1); t(u->d_wsides, u->n_sides + 1); t(u->d_wruns, u->n_runs + 1); t(u->d_jump, u->n_jump + 1);
    if (u->ref_packed) { t(u->d_wref, (n_pos + 3) / 4 + 32); t(u->d_refx, u->n_refx + 1); }
    t(u->d_dhit, nh + 1);
    t(u->d_perm, nh + 1); t(u->d_tfirst, n_tiles + 2); t(u->d_ckey, nh + 1); t(u->d_long, AGX_LONG_MAX);
    t(u->d_tile_cnt, n_tiles + 1); t(u->d_tile_off, n_tiles + 2); t(u->d_cursor, n_tiles + 1);
    t(u->d_words, W_TOTAL);
    t(u->d_chain_end, (size_t)u->n_chain_end + 1);
    t(u->d_node_start, n_pos); t(u->d_node_cnt, n_pos); t(u->d_pos_succ, n_pos); t(u->d_slow_list, n_pos + 64);
    t(u->d_side_pk, n_pos + 2); t(u->d_tile_side, n_tiles + 2); t(u->d_tile_side_start, n_tiles + 2);
    t(u->d_big_list, n_tiles + 1); t(u->d_mid_list, n_tiles + 1);
    t(u->d_scratch, (size_t)AGX_BIG_WAVES * AGX_NF * AGX_MAXV_BIG * 64);
    t(u->d_region_off, n_regions + 1); t(u->d_pool_cnt, n_regions * AGX_REGION_PAD);
    if (u->prm.flags & AGX_FLAG_EDGE_SUPPORT) t(u->d_sup_tot, 2 * n_tiles + 2);
}
template <class U> void list_bufs(U *u, agx_u32 cap, Take &t) { t.note(u->list_cap, cap); t(u->d_unsorted, (size_t)cap + 1); t(u->d_tile_recs, ((size_t)cap + 4) * 8); }      // the tile lists
template <class U> void ovf_bufs(U *u, agx_u32 cap, Take &t) { t.note(u->ovf_cap, cap); t(u->d_ovf, cap); t(u->d_a_ovf, (size_t)cap + 1); if (u->prm.flags & AGX_FLAG_EDGE_SUPPORT) t(u->d_ovf_cnt, cap); }                                  // the edge overflow list
template <class U> void sparse_bufs(U *u, agx_u32 cap, Take &t) { t.note(u->sp_cap, cap); t(u->d_sp_node, (size_t)cap + 1); t(u->d_sp_hop, (size_t)cap + 2); }               // the sparse record table

void do_release(agx_unit *u);


// Capacities of a unit's first build and the HBM they add up to (what do_upload reserves as one block; AlignGraph_amd admits a unit to a device by it:
// agx_unit_hbm_needed).  From the staged counts: positions, hits, runs, conti-mers, read rows.
struct Plan { agx_u32 pool_cap, list_cap, ovf_cap, sp_cap; size_t exact, total; };      // exact: what the five groups take; total: with the room to regrow in and the export's scratch
// The read rows of windows [w_lo, w_hi) of a tile-ordered unit ((0, n_win): all of them), named ONCE for both sides of the upload (agx_forms.h: row_piece): do_upload copies
// what a piece names — bytes of s_codes_t / d_codes, or of s_rowcnt / s_units, entries of s_other_t / d_other — and records ev_rows[w]; the unit's first build expands the same
// piece into d_vcodes behind that event and records ev_win[w] (build_front).  File-order units have none.
RowPiece row_piece(const agx_unit *u, agx_u32 w_lo, agx_u32 w_hi) {
    return row_piece(RowWindows{u->nh, u->stride, u->n_win, u->win_tile, u->s_tfirst.p, u->rows_diffed, u->n_rowcnt, u->s_blockoff.p, u->s_other_t.p, u->n_other_t}, w_lo, w_hi);
}
// Room behind the exact sum, in the same block: a group that proves too small on the device is taken again at its larger size, and while that fits here the unit stays
// in ONE block — it holds no more HBM than it was admitted with, and agx_unit_trim can still give its tail back.  A 64th of the unit; the constant is what small units
// (AGX_TEST_SMALL_CAPS ones above all) regrow in.
inline size_t regrow_slack(size_t exact) { return exact / 64 + (64u << 10) * 100; }
Plan plan_capacities(const agx_unit *u) {
    const size_t n_pos = u->V.n_pos, nh = u->nh;
    Plan P;
    const agx_u32 main_cap = (agx_u32)std::min<size_t>(g_tiny ? n_pos / 8 + 64 : n_pos + n_pos / 4 + 4096, 0xE0000000ull);
    P.pool_cap = u->pool_cap ? u->pool_cap : main_cap + spill_min(u);
    // a hit's arrivals span len - k + 1 positions = 1 + (span - 1) / 64 tiles on average
    const double per_hit = 1.0 + (u->maxlen > u->prm.k ? (double)(u->maxlen - u->prm.k) : 0.0) / AGX_TILE;
    P.list_cap = u->list_cap ? u->list_cap : (agx_u32)std::min<double>(g_tiny ? (double)nh / 2 + 16 : (double)nh * per_hit * 1.1 + 4096, 4.0e9);
    P.ovf_cap = u->ovf_cap ? u->ovf_cap : (g_tiny ? 4u : 1u << 16);
    const size_t ids_cap = n_pos + P.pool_cap;
    P.sp_cap = u->sp_cap ? u->sp_cap : (agx_u32)std::min<size_t>(g_tiny ? 32 : ids_cap / 4 + 4096, 0xFFFFFF00ull);      // special ids: 8 % on the bench unit
    Take m; pool_bufs(u, P.pool_cap, m); fixed_bufs(u, m); list_bufs(u, P.list_cap, m); ovf_bufs(u, P.ovf_cap, m); sparse_bufs(u, P.sp_cap, m);
    P.exact = m.bytes;
    // What AGX_FLAG_EDGE_SUPPORT adds to the groups (d_e_cnt, d_ovf_cnt, d_sup_tot, in Take's alignment) is reserved ON TOP of the block the unit would take without the flag,
    // rounded as a block is: a unit with the flag never plans less than the same unit without it plus its counters, whatever the rounding of blocks does to either sum.
    auto aligned = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t counters = (u->prm.flags & AGX_FLAG_EDGE_SUPPORT) ? aligned((size_t)P.pool_cap * AGX_MAXE * 4) + aligned((size_t)P.ovf_cap * 4) + aligned((2 * (size_t)tiles_of(u) + 2) * 4) : 0;
    const size_t plain = P.exact - counters;
    P.total = plain + regrow_slack(plain) + ((u->prm.flags & AGX_FLAG_KEEP_COUNTS) ? unitig_layout(P.pool_cap, n_pos, P.ovf_cap, nullptr, nullptr, nullptr) : 0);      // (counts are kept for the unitig export)
    if (keeps_paths(u)) P.total += idmap_layout(n_pos + P.pool_cap, P.pool_cap, nullptr, nullptr);      // (a whole-window id map at its worst: every slot a side id and a run)
    if (counters) P.total = round_block(P.total) + counters;
    return P;
}

// Everything a unit holds on the device is taken here, from ONE block of HBM sized by the sum; then the inputs are copied (asynchronously,
// from the staged pinned arrays, on the device's upload stream: behind the copies of the units queued before, beside whatever kernels run on
// the device) and the unit's helper thread is handed what can be prepared meanwhile.  Nothing waits on the host; the unit's first build
// waits for ev_uploaded (on the host) and then expands what was copied.
void do_upload(agx_unit *u) {
    if (u->consumed) throw Error{E_ARG, "one-shot unit: hand its inputs over again before another upload"};
    if (!u->staged) stage_inputs(u);
    if (u->arena.used()) do_release(u);              // uploaded before: start over (the unit's blocks go through the cache)
    u->out.paths.clear(); u->out.paths_ready = false;
    const double t0 = now_ms();
    HIP_OK(hipSetDevice(u->prm.device));
    const size_t n_pos = u->V.n_pos, nh = u->nh;
    u->arena.device = u->prm.device;
    u->n_tiles = tiles_of(u); u->n_regions = regions_of(u);
    const Plan plan = plan_capacities(u);
    u->arena.reserve(plan.total);                        // one block for all of it
    Take t{&u->arena};
    pool_bufs(u, plan.pool_cap, t);                      // (first: what outlives the download lies at the front of the block, agx_unit_trim)
    fixed_bufs(u, t); list_bufs(u, plan.list_cap, t); ovf_bufs(u, plan.ovf_cap, t); sparse_bufs(u, plan.sp_cap, t);
    // the groups took what they were measured to take: a buffer allocated outside them fails here, not later as a silent second block.  Taken later, by design, and not part
    // of the sum: d_huge_list / d_scratch_huge (do_build: a unit that needs pass 3), d_fetch beyond its first 65536 records (fetch_records) — out of the regrowth room or a
    // later block — and d_ut (agx_unit_unitigs), out of the part of `total` that is reserved for it.
    if (u->arena.used() != plan.exact) throw Error{E_DEVICE, "internal: the unit's buffers take " + std::to_string(u->arena.used()) + " bytes, its layout measured " + std::to_string(plan.exact)};
    u->h_words.alloc(W_TOTAL);
    // copies: all of them on the device's upload stream, behind those of the units queued before.  The kernels that expand what was copied
    // (conti-mer tables, vote codes) open the unit's first build instead of following the copies here: a kernel on this stream would wait for
    // CUs while another unit's node sweep holds them all, and every later unit's copies with it.
    DeviceTurn &turn = turn_of(u->prm.device);
    turn.make();
    hipStream_t st = turn.up;
    trace(u, "upload: allocate", t0, n_pos);
    const double tq = now_ms();
    try {
        std::lock_guard<std::mutex> up_turn(turn.up_m);
        u->up_timed = u->ev.all;
        if (u->up_timed) HIP_OK(hipEventRecord(u->ev_up0, st));
        // (AGX_UP_CHUNK_MB: experiment knob — copies cut into pieces of that size)
        static const size_t chunk = getenv("AGX_UP_CHUNK_MB") ? (size_t)atoi(getenv("AGX_UP_CHUNK_MB")) << 20 : 0;
        size_t sent = 0;      // stats.upload_bytes: what the copies below carry
        auto up = [&](void *dst, const void *src, size_t bytes) {
            for (size_t at = 0; at < bytes;) { const size_t m = chunk ? std::min(chunk, bytes - at) : bytes; HIP_OK(hipMemcpyAsync((char *)dst + at, (const char *)src + at, m, hipMemcpyHostToDevice, st)); at += m; }
            sent += bytes;
        };
        up(u->d_segs.p, u->s_segs.p, u->n_segs * sizeof(agx_cmseg)); up(u->d_cntruns.p, u->s_cntruns.p, u->n_cntruns * sizeof(agx_cntrun));
        up(u->d_cntchunks.p, u->s_cntchunks.p, u->n_cntchunks * sizeof(agx_chunk)); up(u->d_segchunks.p, u->s_segchunks.p, u->n_segchunks * sizeof(agx_chunk)); up(u->d_segindex.p, u->s_segindex.p, u->n_segindex * 4);
        if (u->hits_compact) { up(u->d_chits.p, u->s_wire.p, u->n_cblocks * sizeof(agx_chit_block)); up(u->d_cesc.p, u->wire_esc, u->n_cesc * sizeof(agx_whit)); up(u->d_cext.p, u->wire_ext, u->n_cext * 4); }
        else up(u->d_whits.p, !u->tiled ? (const void *)u->s_hits.p : u->s_wire.p ? (const void *)u->s_wire.p : (const void *)u->s_hits_t.p, nh * sizeof(agx_whit));      // (s_wire: the tile-ordered records of a unit that gained nothing from the blocks)
        if (u->sides_compact) { up(u->d_csides.p, u->s_csides.p, u->n_sides * 2); up(u->d_csesc.p, u->wire_listed, u->n_csesc * sizeof(agx_cside_esc)); }
        else up(u->d_wsides.p, u->s_sides.p, u->n_sides * sizeof(agx_wside));
        up(u->d_wruns.p, u->s_runs.p, u->n_runs * sizeof(agx_wrun)); up(u->d_jump.p, u->s_jump_at.p, u->n_jump * 4);
        if (!u->tiled) up(u->d_perm.p, u->s_perm.p, nh * 4);      // (tile-ordered records carry their hit numbers: agx_k_hit_prep writes the array)
        up(u->d_tfirst.p, u->s_tfirst.p, ((size_t)u->n_tiles + 2) * 4);
        HIP_OK(hipEventRecord(u->ev_hits, st));         // what the front of the build needs (conti-mer tables, hit preparation, binning) is there: it starts while the rest still travels
        // The two forms send the same things behind this point and differ in where the read rows go: tile-ordered, the small things first and the rows last, window by window — a
        // window's sweep starts when its rows are in (do_build); in file order the rows first, whole.
        auto small = [&] {      // the listed bases (first needed by the sweep), the unit sequence, the chain ends (first needed by the walk preparation), the region layout
            up(u->d_other.p, u->tiled ? u->s_other_t.p : u->s_other.p, others_up(u) * 8);
            if (u->ref_packed) { up(u->d_wref.p, u->s_ref.p, (n_pos + 3) / 4); up(u->d_refx.p, u->s_refx.p, u->n_refx * sizeof(agx_refx)); } else up(u->d_ref.p, u->s_ref.p, n_pos);
            up(u->d_chain_end.p, u->s_chain_end.p, (size_t)u->n_chain_end * 4);
            layout_regions(u, nullptr, u->pool_cap - spill_min(u), true, st, &sent);      // (equal shares always fit)
        };
        auto tables = [&] { up(u->d_blockoff.p, u->s_blockoff.p, u->n_blockoff * 4); up(u->d_blockfirst.p, u->s_blockfirst.p, u->n_blockfirst * 4); up(u->d_anchor.p, u->s_anchor.p, u->n_anchor * 4); };      // of rows that cross as differences
        if (u->tiled) {
            small();
            if (u->rows_diffed) tables();
            for (agx_u32 w = 0; w < u->n_win; w++) {      // window w's piece of the rows, then its event
                const RowPiece p = row_piece(u, w, w + 1);
                if (u->rows_diffed) { up(u->d_rowcnt.p + p.cnt_lo, u->s_rowcnt.p + p.cnt_lo, p.cnt_hi - p.cnt_lo); up(u->d_units.p + p.unit_lo, u->s_units.p + p.unit_lo, (p.unit_hi - p.unit_lo) * 2); }
                else up(u->d_codes.p + p.code_lo, u->s_codes_t.p + p.code_lo, p.code_hi - p.code_lo);
                HIP_OK(hipEventRecord(u->ev_rows[w], st));
            }
        } else {
            if (u->rows_diffed) { up(u->d_units.p, u->s_units.p, u->n_units * 2); up(u->d_rowcnt.p, u->s_rowcnt.p, u->n_rowcnt); tables(); }
            else up(u->d_codes.p, u->s_codes.p, u->n_codes);
            small();
        }
        HIP_OK(hipEventRecord(u->ev_uploaded, st));
        u->stats.upload_bytes = sent;
    } catch (...) { (void)hipStreamSynchronize(st); throw; }      // (copies that were queued before the failure must not outlive the unit's HBM block)
    u->expanded = false;
    trace(u, "upload: queue copies", tq, n_pos);
    // While the copies run: the download's pinned buffers, by estimate (helper_estimate), on a helper
    // thread.  Mapping and registering them costs 5-13 ms for a cold cache.  Between the build and the download that was on the unit's critical
    // path; on the unit's worker right here it kept the NEXT unit's upload from starting (a job hands its units out one at a time); beside the
    // build's kernels, or at the start of do_build, it held up the other units' HIP calls.  do_download joins the helper and re-sizes what is too small.
    auto dl_buffers = [u, n_pos] {
        static std::mutex one_at_a_time;      // five units pinning memory at once take five times as long each, and stall everything else that touches the address space
        std::lock_guard<std::mutex> l(one_at_a_time);
        const double th0 = now_ms();
        try {
            if (hipSetDevice(u->prm.device) != hipSuccess) return;
            graph_arrays(u, helper_estimate(n_pos), [](int, auto &h, auto &, size_t n, size_t pad) { h.alloc(n + pad); });
        } catch (...) { }                               // do_download allocates what is missing and reports
        trace(u, "helper: download buffers", th0, n_pos);
    };
    if (!(u->prm.flags & AGX_FLAG_ONE_SHOT)) u->helper.submit(UnitHelper::DL, dl_buffers);      // (a one-shot unit's download borrows the staged inputs' memory: nothing to pin)
    start_helper(u);                                     // then the output buffers

    u->uploaded = true; u->built = false; u->downloaded = false; u->support_valid = false;
    if (!u->pending_walk) { u->pending_walk = true; g_walks_pending.fetch_add(1); }
    u->stats.ms_upload = now_ms() - t0;
    u->stats.device_bytes = u->arena.capacity();
    u->stats.rows_by_reference = u->rows_diffed ? (uint32_t)((u->tiled ? u->nh : u->n_rows) - u->n_rows_explicit) : 0u;
}

// The three output buffers of a unit: reserved by estimate (the walk grows what is too small), every page touched, the initial contigs
// copied.  A 30 Mb unit's outputs are 100 MB of fresh memory: faulted in inside the walk and after it they cost 8-10 ms of the unit's
// critical path, and 20 ms on the unit's own worker before the build (five workers faulting at once).  So a helper thread makes them while
// the unit is uploaded and built; agx_unit_finish joins it.
void prepare_outputs(agx_unit *u) {
    if (u->out_ready) return;
    // a few at a time: with huge pages five threads touching fresh memory at once cost each other 20 % (tests/tools/faultbench.cpp), but 24 units
    // taking strict turns made the last small units of a cfg5s job wait 3 ms for buffers that take 1 ms to make
    struct Slots { std::mutex m; std::condition_variable cv; int free = 4; } static slots;
    { std::unique_lock<std::mutex> l(slots.m); slots.cv.wait(l, [] { return slots.free > 0; }); slots.free--; }
    struct Give { ~Give() { { std::lock_guard<std::mutex> l(slots.m); slots.free++; } slots.cv.notify_one(); } } give;
    try {
        const size_t n_pos = u->V.n_pos;
        u->out.pre_extended.n = 0; u->out.extended.n = 0; u->out_initial.n = 0;
        u->out.pre_extended.reserve(n_pos + n_pos / 8 + 8192); u->out.pre_extended.prefault();
        u->out.extended.reserve(n_pos + n_pos / 16 + 4096); u->out.extended.prefault();
        u->out_initial.reserve(u->V.n_initial);                      // (one copy: a 30 Mb unit's initial contigs are 30 MB)
        if (u->V.n_initial) u->out_initial.append(u->V.initial, u->V.n_initial);
        u->out_ready = true;
    } catch (...) { u->out_ready = false; }                              // out of memory: agx_unit_finish tries again on its own thread and reports
}
void join_helper(agx_unit *u) { u->helper.wait(UnitHelper::OUT); }
void join_dl_helper(agx_unit *u) { u->helper.wait(UnitHelper::DL); }
void drop_outputs(agx_unit *u) { join_helper(u); u->out_ready = false; }
void start_helper(agx_unit *u) {
    join_helper(u);
    if (u->out_ready) return;
    u->helper.submit(UnitHelper::OUT, [u] { const double th0 = now_ms(); prepare_outputs(u); trace(u, "helper: output buffers", th0, u->V.n_pos); });      // (no helper: finish prepares the outputs itself)
}

// The three exclusive scans of a build (0: the tile histogram, 1: the side counts per tile, 2: the special ids per word), by the one-launch form with the scan's own
// descriptors or — no descriptors — by the three-launch form over d_scan_tmp (AGX_SCAN_LEGACY)
inline unsigned long long *scan_desc(agx_unit *u, int which) { return g_scan1 ? u->d_scan_desc.p + which * u->scan_desc_n : nullptr; }
inline void queue_scan(agx_unit *u, const agx_u32 *in, agx_u32 *out, agx_u32 n, int which, hipStream_t st) {
    if (unsigned long long *desc = scan_desc(u, which)) agx_launch_exclusive_scan1(in, out, n, desc, st); else agx_launch_exclusive_scan(in, out, n, u->d_scan_tmp.p, st);
}
// What queue_walk_prep assumes zeroed (see there): segments `at` .. `at + 3` of the caller's ONE zeroing launch (first_scan: with scan 0's descriptors, a build's) and the
// fill of a_mark: two commands.
void queue_zero(agx_unit *u, agx_zero_args &Z, int at, bool first_scan, hipStream_t st) {
    auto seg = [&](void *ptr, size_t words) { Z.p[at] = (agx_u32 *)ptr; Z.n[at++] = (agx_u32)words; };
    seg(u->d_tile_side.p + u->n_tiles, 1); seg(u->d_sp_cnt.p, (size_t)u->n_words + 1);
    seg(u->d_scan_desc.p + (first_scan ? 0 : u->scan_desc_n), (first_scan ? 6 : 4) * u->scan_desc_n); seg(u->d_sp_bits.p, 2 * ((size_t)u->n_words + 1));
    agx_launch_zero(&Z, st); HIP_OK(hipMemsetAsync(u->d_a_mark.p, 0, u->V.n_pos + u->pool_cap + 2, st));
}
// The tail of a build's and a reprune's verdict: more special ids than the sparse record table holds — it is taken again, larger, and the caller goes round again (true) —,
// or the unit's ids and special ids are counted.
bool walk_ids_verdict(agx_unit *u, const agx_u32 *w) {
    if (w[W_N + 2] > u->sp_cap) { Take grow{&u->arena}; sparse_bufs(u, w[W_N + 2] + w[W_N + 2] / 8 + 1024, grow); return true; }
    const unsigned long long ids = (unsigned long long)u->V.n_pos + w[W_N + 1];
    if (ids >= 0xFFFFFF00ull) throw Error{E_OVERFLOW, "walk graph exceeds 2^32 ids"};
    u->n_ids = (agx_u32)ids; u->n_special = w[W_N + 2]; return false;
}

// The back of a build behind its edge passes, and all of a reprune behind its kernel: the walk preparation over the side counts in side_pk / tile_side (side counts ->
// scan -> walk ids, node records, rewritten edges, forced-run flags -> special ids with the stream cuts), then the counters to the host by a kernel at the end of the chain
// and the event their reader waits for.  before_counters: what the caller records between the two (a build: its section mark and the device's build_done event).
// Assumes zeroed: a_mark (agx_k_assign_aid and agx_k_emit_alive only ever store 1), sp_bits and sp_cnt (agx_k_special_bits writes the words of the live ids only),
// tile_side[n_tiles] (the scan's closing entry) and the descriptors of the two scans.  Every other array it writes it writes for every live id, node or special record.
template <class F> void queue_walk_prep(agx_unit *u, hipStream_t st, F before_counters) {
    const agx_u32 n_pos = (agx_u32)u->V.n_pos;
    agx_compact_args C; memset(&C, 0, sizeof C);
    C.node_start = u->d_node_start.p; C.node_cnt = u->d_node_cnt.p; C.n_flags = u->d_flags.p; C.n_base = u->d_base.p;
    C.nk_off0 = u->d_off0.p; C.n_sref = u->d_sref.p; C.n_next = u->d_next.p; C.ref = u->d_ref.p; C.n_pos = n_pos;
    C.side_pk = u->d_side_pk.p; C.tile_side_start = u->d_tile_side_start.p; C.aid_of = u->d_aid_of.p;
    C.a_str = u->d_a_str.p; C.a_meta = u->d_a_meta.p; C.a_nid = u->d_a_nid.p; C.ovf = u->d_ovf.p; C.n_ovf = 0; C.a_ovf = u->d_a_ovf.p;
    C.abort = u->d_words.p + W_STATUS;
    C.a_mark = u->d_a_mark.p; C.side_xpos = u->d_side_xpos.p; C.sparse_min = (u->prm.flags & AGX_FLAG_SPARSE_MIN) ? 1u : 0u;
    C.sp_bits = u->d_sp_bits.p; C.sp_cnt = u->d_sp_cnt.p; C.sp_rank = u->d_sp_rank.p; C.sp_node = u->d_sp_node.p; C.sp_cap = u->sp_cap;
    C.segs = u->d_segs.p; C.n_seg0 = u->n_seg0; C.cm_start = u->d_cm_start.p; C.sp_hop = u->d_sp_hop.p; C.seg_index = u->d_segindex.p;
    queue_scan(u, u->d_tile_side.p, u->d_tile_side_start.p, u->n_tiles, 1, st);      // per tile: the sweep has scanned inside the tiles
    agx_launch_compact(&C, u->d_chain_end.p, u->n_chain_end, u->d_words.p + W_OVFCOUNT, u->ovf_cap, st);
    AGX_CHECKPOINT("compact");
    u->cuts = stream_cuts(n_pos); u->cuts.cut_out = u->d_words.p + W_CUT;
    agx_launch_special(&C, u->n_words, u->d_sp_rank.p, u->d_scan_tmp.p, scan_desc(u, 2),
                       u->d_words.p + W_N, u->d_tile_off.p + u->n_tiles, u->d_tile_side_start.p + u->n_tiles, u->d_pool_cnt.p, u->n_regions, u->d_words.p + W_POOL, u->cuts.n ? &u->cuts : nullptr, st);
    u->walk_args = C;
    AGX_CHECKPOINT("special");
    before_counters();
    {   void *dst = u->h_words.dev(); const void *src = u->d_words.p; const size_t bytes = W_TOTAL * 4;      // the counters, by a kernel at the end of the chain (a copy
        agx_launch_copy_out(&dst, &src, &bytes, 1, st); }                                                              // command would queue behind the uploads on the copy engines)
    HIP_OK(hipEventRecord(u->ev_built, st));
}

// All kernels of one build are queued back to back with the current buffer capacities; the counters they produce (tile-list entries, nodes, overflowed tiles, edge overflow,
// side variants) are read after ONE synchronisation.  A capacity that proved too small is grown and the build repeats — the first guesses (do_upload) make that rare.  An
// attempt is the stages below, queued in this order by do_build under the device's turn; each stage's head names the stream it queues on, the events it waits for and
// records, and what it takes to be in HBM.  What an attempt is planned by, when it takes the turn:
struct Attempt { DeviceTurn &turn;
    bool early;      // a unit's first build starts on the arrays that arrive first (ev_hits); the read bases are waited for on the device, in front of their first use (not in builds that time their sections: those would time the wait)
    bool windows;    // r06: a tile-ordered unit's first build expands its read rows and sweeps its tiles WINDOW BY WINDOW, each when its piece of the upload (RowPiece) has landed: the sweep of the unit's front runs beside the upload of its back
    agx_u32 n_win;   // in so many windows (a build that has waited for the whole upload on the host — timed sections — has nothing to overlap: one window, no boundaries to pay for)
    double t_queue; hipEvent_t trace_from; };      // host time when the turn was asked for; AGX_TRACE_GAP: the end of the device's previous sweep
// WAIT AND TAKE THE TURN.  Host: waits for ev_hits (early) or ev_uploaded — the build streams are shared by all units of the device: nothing that could wait long is queued
// on them —, then locks the device's turn: no other stage does, and do_build unlocks it behind the attempt's last command.  Front stream: waits for the previous build's
// sweep_done (build_done where either build times its sections): a front may run beside that build's edge passes and walk preparation, not beside its sweep.
std::unique_lock<std::mutex> build_take_turn(agx_unit *u, int attempt, Attempt &A) {
    const double tb0 = now_ms(); DeviceTurn &turn = A.turn;
    A.early = !u->expanded && attempt == 0 && !u->ev.all; A.windows = !u->expanded && u->tiled; A.n_win = (A.windows && A.early) ? u->n_win : 1u;
    HIP_OK(wait_event(A.early ? u->ev_hits : u->ev_uploaded));
    trace(u, "build: wait for upload", tb0, u->V.n_pos);
    A.t_queue = now_ms();
    std::unique_lock<std::mutex> my_turn(turn.m);
    if (turn.n) HIP_OK(hipStreamWaitEvent(turn.front, (u->ev.all || turn.prev_exclusive) ? turn.build_done[(turn.n - 1) & 1] : turn.sweep_done[(turn.n - 1) & 1], 0));
    return my_turn;
}
// FRONT, all of it on the front stream.  In HBM: what ev_hits stands for (hit, side and run records, conti-mer runs, tile_first).  An early build also waits for ev_uploaded
// (file order) or ev_rows[0] (tile order: the reference, the listed bases and the region layout travel in front of the first rows), then for ev_rows[w] in front of window
// w's rows.  Queues a first build's expansions out of the wire forms, the zeroing, hit_prep, the scan of the tile histogram, the tile lists, the reference and the file-order
// rows; records ev_front; then expands the tile-ordered rows piece by piece and records ev_win[w] behind each.
void build_front(agx_unit *u, const Attempt &A) {
    hipStream_t st = A.turn.front; const agx_u32 n_pos = (agx_u32)u->V.n_pos, nh = (agx_u32)u->nh;
    if (u->ev.all) HIP_OK(hipEventRecord(u->ev.first, st));      // (every event record costs the stream a few microseconds: untimed builds record only what orders them)
    if (!u->expanded) {   // the unit's first build: the hits and runs out of their wire forms, then the conti-mer tables from their runs (agx_cmseg: count per position, scan, keys, heads); the read bases follow behind the binning
        if (u->hits_compact) agx_launch_expand_hits(u->d_chits.p, u->d_cesc.p, u->d_cext.p, u->d_whits.p, nh, u->maxlen, st);
        if (u->sides_compact) agx_launch_expand_sides(u->d_csides.p, u->d_csesc.p, (agx_u32)u->n_csesc, u->d_wsides.p, (agx_u32)u->n_sides, u->side_first, u->d_cside_scan.p, st);
        agx_launch_expand_runs(u->d_wruns.p, u->d_runs.p, (agx_u32)u->n_runs, st);
        agx_launch_cm_tables(u->d_cntruns.p, u->d_cntchunks.p, (agx_u32)u->n_cntchunks, u->d_segs.p, u->d_segchunks.p, (agx_u32)u->n_segchunks, u->d_cm_start.p, u->d_cm.p, u->d_cm_head.p, n_pos, (agx_u32)u->n_cm, st);
    }
    agx_zero_args Z; memset(&Z, 0, sizeof Z);
    Z.p[0] = u->d_words.p; Z.n[0] = W_TOTAL; Z.p[1] = u->d_tile_cnt.p; Z.n[1] = u->n_tiles + 1; Z.p[2] = u->d_cursor.p; Z.n[2] = u->n_tiles + 1; Z.p[3] = u->d_pool_cnt.p; Z.n[3] = u->n_regions * AGX_REGION_PAD;
    queue_zero(u, Z, 4, true, st);
    u->ev.begin(); u->ev.mark(B_START, st);
    agx_prep_args PA{(const agx_whit *)u->d_whits.p, (const agx_wside *)u->d_wsides.p, u->d_runs.p, u->d_dhit.p, nh, u->prm.k, n_pos, u->d_tile_cnt.p, u->d_words.p + W_ERR,
                     u->d_perm.p, u->d_tfirst.p, u->d_ckey.p, u->lookback, u->d_long.p, u->d_words.p + W_LONGCOUNT, u->tiled ? 1u : 0u, u->d_perm.p};
    agx_launch_hit_prep(&PA, st);
    AGX_CHECKPOINT("hit_prep");
    u->ev.mark(B_PREP, st);
    queue_scan(u, u->d_tile_cnt.p, u->d_tile_off.p, u->n_tiles, 0, st);
    agx_fill_args FA{u->d_tile_off.p, u->d_tfirst.p, u->d_perm.p, u->d_ckey.p, u->d_dhit.p, u->d_runs.p, u->d_tile_recs.p, u->d_unsorted.p, u->n_tiles, u->list_cap, u->prm.k, u->lookback,
                     u->d_long.p, u->d_words.p + W_LONGCOUNT, u->d_words.p + W_ERR, u->d_words.p + W_STATUS, u->dense ? 1u : 0u};
    agx_launch_tile_fill(&FA, st);                  // every tile's list from its window of the tile order
    if (u->dense) {                                 // the fallback for a unit with more long hits than a list's window scan takes: queued once a build has met them (an idle launch of a kernel per tile costs 0.1 ms)
        agx_bin_args BA{u->d_dhit.p, nh, u->d_tile_off.p, u->d_cursor.p, u->d_unsorted.p, u->list_cap, u->d_words.p + W_LONGCOUNT};
        agx_launch_bin_fill(&BA, st);
        agx_launch_tile_sort(&FA, st);
    }
    AGX_CHECKPOINT("tile_sort");
    if (!u->expanded) {   // the vote codes (and the region layout, the last copy of the upload) are first needed by the sweep
        if (!u->tiled) {  // the file-order forms: no windows, the rows whole with their listed bases
            if (A.early) HIP_OK(hipStreamWaitEvent(st, u->ev_uploaded, 0));      // (at most the tail of this unit's own upload: a build stream never waits for anything else)
            if (u->rows_diffed) agx_launch_expand_rows(u->d_whits.p, nh, u->d_wsides.p, u->d_wruns.p, u->d_anchor.p, u->d_blockfirst.p, u->d_rowcnt.p, u->d_blockoff.p, u->d_units.p, u->d_wref.p, u->d_vcodes.p, u->n_rows, u->stride, u->d_other.p, u->n_other, st);
            else agx_launch_expand_codes(u->d_codes.p, u->d_vcodes.p, (codes_bytes(u) * 4 + 15) / 16 * 16, u->d_other.p, u->n_other, st);
        } else if (A.early) HIP_OK(hipStreamWaitEvent(st, u->ev_rows[0], 0));
        if (u->ref_packed) agx_launch_expand_ref(u->d_wref.p, u->d_ref.p, ((size_t)n_pos + 15) / 16 * 16, u->d_refx.p, (agx_u32)u->n_refx, st);      // (the letters are first read by the sweep's write-out)
        u->expanded = true;
    }
    HIP_OK(hipEventRecord(u->ev_front, st));
    for (agx_u32 w = 0; A.windows && w < A.n_win; w++) {      // behind ev_front: the rows of window w out of their upload form when they are in, then the listed bases among them
        const RowPiece p = A.n_win == 1 ? row_piece(u, 0, u->n_win) : row_piece(u, w, w + 1);
        if (A.early && w) HIP_OK(hipStreamWaitEvent(st, u->ev_rows[w], 0));
        if (p.r_hi > p.r_lo) {
            if (u->rows_diffed) agx_launch_expand_rows(u->d_whits.p, nh, u->d_wsides.p, u->d_wruns.p, u->d_anchor.p, u->d_blockfirst.p + p.blk_lo, u->d_rowcnt.p + p.cnt_lo, u->d_blockoff.p + p.blk_lo, u->d_units.p, u->d_wref.p,
                                                       u->d_vcodes.p + p.v_lo, (agx_u32)(p.r_hi - p.r_lo), u->stride, nullptr, 0, st);      // (every row's anchor is its own hit: the anchor bits are all ones)
            else agx_launch_expand_codes(u->d_codes.p + p.code_lo, u->d_vcodes.p + p.v_lo, p.v_hi - p.v_lo, nullptr, 0, st);
            agx_launch_patch_codes(u->d_other.p + p.o_lo, p.o_hi - p.o_lo, u->d_vcodes.p, st);
        }
        HIP_OK(hipEventRecord(u->ev_win[w], st));
    }
}
// SWEEP, all of it on the main stream.  Waits for ev_front (the lists, the reference, file-order or resident rows) and for ev_win[w] in front of window w's tiles.  Queues
// pass 0 — every tile with small LDS buckets — per window between ev_sw0[w] and ev_sw1[w], records the device's sweep_done (the next build's front may start), then the
// tiles that overflowed: with wider buckets and, once a build has met such a tile, with global scratch (device-side lists).
void build_sweep(agx_unit *u, Attempt &A) {
    hipStream_t st = A.turn.main; HIP_OK(hipStreamWaitEvent(st, u->ev_front, 0)); u->ev.mark(B_BIN, st);
    agx_node_kargs K; fill_node_args(u, K);
    for (agx_u32 w = 0; w < A.n_win; w++) {
        K.tile_lo = A.n_win == 1 ? 0u : u->win_tile[w]; K.tile_hi = A.n_win == 1 ? u->n_tiles : u->win_tile[w + 1];
        if (A.windows) { HIP_OK(hipStreamWaitEvent(st, u->ev_win[w], 0)); HIP_OK(hipEventRecord(u->ev_sw0[w], st)); }      // (behind the wait: the sweep's time must not hold the rows' journey)
        agx_launch_node_sweep(&K, st);
        if (A.windows) HIP_OK(hipEventRecord(u->ev_sw1[w], st));
    }
    AGX_CHECKPOINT("node_sweep");
    u->ev.mark(B_NODE, st); u->stats.node_sweep_launches++;
    A.trace_from = A.turn.prev_node; A.turn.prev_node = u->ev.e[B_NODE]; HIP_OK(hipEventRecord(A.turn.sweep_done[A.turn.n & 1], st));
    agx_launch_node_sweep_big(&K, st);      // the two fallback passes: they find their (usually empty) tile lists on the device.  A unit is built once, so they
    if (u->huge) agx_launch_node_sweep_huge(&K, st);
    AGX_CHECKPOINT("node_sweep_big");       // are always queued: two idle launches cost less than repeating the build of a unit that turns out to need them
    u->ev.mark(B_BIG, st);
}
// EDGES: passes A and B on the main stream.  Passes J and B insert edges out of different sources (positions with one variant / with several) and both wait on memory more
// than they compute: J goes to the front stream, behind pass A (ev_passA) and in front of the next build's front, and runs beside B; the main stream waits for it (ev_passJ)
// behind B.  Timed builds and AGX_DEBUG_SYNC keep all three on the main stream.
void build_edges(agx_unit *u, const Attempt &A) {
    hipStream_t st = A.turn.main, front = A.turn.front;
    agx_edge_kargs E; fill_edge_args(u, E);
    const bool side_j = !u->ev.all && !g_debug_sync;
    agx_launch_edge_sweep(&E, st);
    AGX_CHECKPOINT("edge_sweep");
    if (side_j) {
        HIP_OK(hipEventRecord(u->ev_passA, st)); HIP_OK(hipStreamWaitEvent(front, u->ev_passA, 0));
        agx_launch_edge_jump(&E, front);
        HIP_OK(hipEventRecord(u->ev_passJ, front));
    } else { agx_launch_edge_jump(&E, st); AGX_CHECKPOINT("edge_jump"); }
    u->ev.mark(B_EDGE, st);
    agx_launch_edge_slow(&E, st);
    AGX_CHECKPOINT("edge_slow");
    u->ev.mark(B_SLOW, st);
    if (side_j) HIP_OK(hipStreamWaitEvent(st, u->ev_passJ, 0));
}
// VERDICT, on the host behind ev_built, over the counters in h_words: throws the input's and the internal errors; grows the ONE capacity that proved too small (the arena
// keeps the old buffer) and says "again" (true), or stores the unit's counts.  Whatever a retry changes on the device goes through the download
// stream and a fresh ev_uploaded — recorded only here — which the next attempt waits for.
bool build_verdict(agx_unit *u, const Attempt &A, int attempt) {
    hipStream_t down = A.turn.down; const agx_u32 *w = u->h_words.p;
    if (w[W_ERR] & 1u) throw Error{E_ALIGNMENT, "BOWTIE ALIGNMENT ERROR"};
    if (w[W_ERR] & 2u) throw Error{E_UNSUPPORTED, "read alignment beyond the end of the unit sequence"};
    if (w[W_ERR] & (4u | 8u)) throw Error{E_DEVICE, (w[W_ERR] & 4u) ? "internal: the staged order of the hits is not the order of their first tiles" : "internal: a tile's list does not hold what its histogram counted"};
    u->n_tile_entries = w[W_N];
    bool again = true; Take grow{&u->arena};
    if ((w[W_STATUS] & 16u) && !u->dense) u->dense = true;      // more long hits than the window scan takes: again, with the scatter fallback queued
    else if (u->n_tile_entries > u->list_cap) list_bufs(u, u->n_tile_entries + u->n_tile_entries / 8 + 1024, grow);
    else if ((w[W_STATUS] & 2u) && !u->huge) {     // a position beyond the 64 variants of pass 2 (deep repeats under a wide --distanceHigh): queue pass 3 and build again
        u->huge = true; u->d_huge_list.alloc(u->arena, (size_t)u->n_tiles + 1); u->d_scratch_huge.alloc(u->arena, (size_t)AGX_HUGE_WAVES * AGX_NF * AGX_MAXV_HUGE * 64);
    } else if (w[W_STATUS] & 2u) throw Error{E_OVERFLOW, "more than " + std::to_string(AGX_MAXV_HUGE) + " node variants at one position"};
    else if (w[W_STATUS] & 1u) {                   // the node pool ran out: cut the slices to what the regions asked for
        std::vector<agx_u32> padded((size_t)u->n_regions * AGX_REGION_PAD), demand(u->n_regions);
        HIP_OK(hipMemcpyAsync(padded.data(), u->d_pool_cnt.p, padded.size() * 4, hipMemcpyDeviceToHost, down)); HIP_OK(hipStreamSynchronize(down));
        for (agx_u32 r = 0; r < u->n_regions; r++) demand[r] = padded[(size_t)r * AGX_REGION_PAD];
        const unsigned long long need = layout_regions(u, demand.data(), 0, false, down);
        if (need >= 0xFFFFFF00ull) throw Error{E_OVERFLOW, "node table exceeds 2^32 entries"};
        if (need > u->pool_cap) pool_bufs(u, (agx_u32)need, grow);
        layout_regions(u, demand.data(), 0, true, down);
    } else if (w[W_OVFCOUNT] > u->ovf_cap) ovf_bufs(u, w[W_OVFCOUNT] + w[W_OVFCOUNT] / 2 + 1024, grow);
    else again = walk_ids_verdict(u, w);
    if (again) { HIP_OK(hipEventRecord(u->ev_uploaded, down)); return true; }
    u->n_nodes = w[W_POOL]; u->n_big = w[W_BIGCOUNT]; u->n_mid = w[W_MIDCOUNT]; u->n_ovf = w[W_OVFCOUNT]; u->n_slow = w[W_SLOWCOUNT];
    u->stats.build_attempts = (uint32_t)attempt + 1; u->stats.n_spilled = w[W_SPILL]; u->stats.dense_lists = w[W_LONGCOUNT] > AGX_LONG_MAX ? 2u : w[W_LONGCOUNT] ? 1u : 0u;
#ifdef AGX_SWEEP_STATS
    {   const agx_u32 *c = w + W_N + 6;
        fprintf(stderr, "[agx sweep stats] wave-entries %u (lanes with an arrival %u = %.1f per entry); leave the fast path: %u entries / %u lanes; of those not a first store: %u / %u; "
                        "variant 0 incompatible: %u / %u; several candidate keys: %u / %u; entries with a multi-run record %u\n",
                c[0], c[3], c[0] ? (double)c[3] / c[0] : 0.0, c[4], c[5], c[6], c[7], c[8], c[9], c[10], c[11], c[12]); }
#endif
    return false;
}
// STATISTICS of a converged build, from its last attempt's events
void build_stats(agx_unit *u, const Attempt &A) {
    u->stats.ms_build_span = u->ev.all ? u->ev.span() : 0.0;
    u->stats.ms_prep = u->ev.ms(B_PREP); u->stats.ms_bin = u->ev.ms(B_BIN); u->stats.ms_node_sweep = u->ev.ms(B_NODE);
    if (A.windows) {      // the sweep's time is the sum over its windows (between them the stream may have waited for rows that were still travelling)
        u->stats.ms_node_sweep = 0; for (agx_u32 w = 0; w < A.n_win; w++) { float f = 0; if (hipEventElapsedTime(&f, u->ev_sw0[w], u->ev_sw1[w]) == hipSuccess) u->stats.ms_node_sweep += f; else (void)hipGetLastError(); } }
    u->stats.ms_node_big = u->ev.ms(B_BIG); u->stats.ms_edge_fast = u->ev.ms(B_EDGE); u->stats.ms_edge_slow = u->ev.ms(B_SLOW); u->stats.ms_edge_sweep = u->stats.ms_edge_fast + u->stats.ms_edge_slow; u->stats.ms_compact = u->ev.ms(B_COMPACT);
    if (u->up_timed) { float f = 0; if (hipEventElapsedTime(&f, u->ev_up0, u->ev_uploaded) == hipSuccess) u->stats.ms_upload_dev = f; else (void)hipGetLastError(); }
}
void do_build(agx_unit *u) {
    if (!u->uploaded) do_upload(u);
    HIP_OK(hipSetDevice(u->prm.device));
    u->stats.node_sweep_launches = u->stats.edge_sweep_launches = 0;
    u->support_valid = false; u->stats.n_support_events = 0;      // (the edge counters are the last build's: counted again on the next request)
    DeviceTurn &turn = turn_of(u->prm.device);
    for (int attempt = 0;; attempt++) {
        if (attempt > 8) throw Error{E_DEVICE, "build did not converge"};
        Attempt A{turn, false, false, 1u, 0.0, nullptr};
        std::unique_lock<std::mutex> my_turn = build_take_turn(u, attempt, A);
        build_front(u, A); build_sweep(u, A); build_edges(u, A);
        queue_walk_prep(u, turn.main, [&] {      // WALK PREPARATION, main stream; records build_done, ev_built
            u->ev.mark(B_COMPACT, turn.main); u->stats.edge_sweep_launches++;
            if (u->ev.all) HIP_OK(hipEventRecord(u->ev.last, turn.main));
            HIP_OK(hipEventRecord(turn.build_done[turn.n & 1], turn.main));               // (a stream wait binds to the record that precedes it: the handle may be recorded again later)
        });
        turn.n++; turn.prev_exclusive = u->ev.all;
        my_turn.unlock();
        trace(u, "build: queue kernels", A.t_queue, u->V.n_pos);
        const double tb2 = now_ms();
        HIP_OK(wait_event(u->ev_built)); HIP_OK(hipGetLastError());
        trace(u, "build: wait for kernels", tb2, u->V.n_pos);
        if (g_trace_gap && A.trace_from && A.trace_from != u->ev.e[B_NODE]) {      // diagnostic (units must outlive each other's builds): end of the previous sweep -> start of this one
            float f = 0; if (hipEventElapsedTime(&f, A.trace_from, u->ev.e[B_BIN]) == hipSuccess) fprintf(stderr, "[agx gap] %.3f ms between sweeps, %.3f ms sweep\n", f, u->ev.ms(B_NODE)); else (void)hipGetLastError(); }
        if (build_verdict(u, A, attempt)) continue;
        u->built = true; u->downloaded = false; u->trimmed = false; u->front_windows = A.n_win;
        return build_stats(u, A);
    }
}

void stream_wait_all(agx_unit *u);

// The prune of a built unit at another coverage (agx_unit_reprune).  Coverage decides AGX_NF_DEAD and what follows from it — the side counts and the walk
// preparation —, nothing else of a build: one kernel rewrites the bit and the side counts from the per-node coverage the unit kept (agx_k_reprune), then the build's own
// tail runs again (queue_walk_prep).  It takes the device's turn and the main build stream like a build, and waits for its own counters.  Cleared first: only what the walk
// preparation counts into or marks (a build's agx_launch_zero clears that among everything else); W_POOL, W_OVFCOUNT, the region counters and W_STATUS are the
// converged build's and are read again.  Lowering the threshold makes more special ids: the sparse record table grows as in the build's retry loop.
void do_reprune(agx_unit *u, uint32_t coverage) {
    const double t0 = now_ms();
    if (!(u->prm.flags & AGX_FLAG_KEEP_COUNTS)) throw Error{E_ARG, "reprune: the unit was created without AGX_FLAG_KEEP_COUNTS (the per-node coverage stays on the device only with it)"};
    if (coverage > 0x7FFFFFFFu) throw Error{E_ARG, "reprune: coverage above 2^31 - 1 (the prune compares signed numbers)"};
    if (!u->built || u->trimmed) throw Error{E_ARG, "reprune: the unit is not built (call agx_unit_build; not after agx_unit_trim or agx_unit_release)"};
    if ((u->prm.flags & AGX_FLAG_ONE_SHOT) && (u->consumed || u->downloaded)) throw Error{E_ARG, "reprune: a one-shot unit is re-pruned before its download or finish (its landing memory is used once)"};
    HIP_OK(hipSetDevice(u->prm.device));
    stream_wait_all(u);                              // (no download of the old walk graph is on its way)
    join_helper(u);
    u->out.paths.clear(); u->out.paths_ready = false;      // the kept stretches name the old walk ids
    const agx_u32 n_pos = (agx_u32)u->V.n_pos;
    DeviceTurn &turn = turn_of(u->prm.device);
    struct Failed { agx_unit *u; bool armed; ~Failed() { if (armed) u->built = false; } } failed{u, true};      // (an error behind the first launch leaves flags nobody has counted: the next build makes them again)
    for (int attempt = 0;; attempt++) {
        if (attempt > 2) throw Error{E_DEVICE, "reprune did not converge"};
        {
            std::unique_lock<std::mutex> my_turn(turn.m);
            hipStream_t st = turn.main;
            agx_zero_args Z; memset(&Z, 0, sizeof Z);
            Z.p[0] = u->d_words.p + W_N; Z.n[0] = W_TOTAL - W_N;
            queue_zero(u, Z, 1, false, st);
            agx_reprune_args R; memset(&R, 0, sizeof R);
            R.node_start = u->d_node_start.p; R.node_cnt = u->d_node_cnt.p; R.nk_cid = u->d_cid.p; R.n_counts = u->d_counts.p; R.n_flags = u->d_flags.p;
            R.side_pk = u->d_side_pk.p; R.tile_side = u->d_tile_side.p; R.n_pos = n_pos; R.pool_cap = u->pool_cap; R.coverage = (int)coverage; R.abort = u->d_words.p + W_STATUS;
            agx_launch_reprune(&R, u->n_tiles, st);
            AGX_CHECKPOINT("reprune");
            queue_walk_prep(u, st, [] {});
        }
        HIP_OK(wait_event(u->ev_built));
        HIP_OK(hipGetLastError());
        const agx_u32 *w = u->h_words.p;
        if (w[W_STATUS]) throw Error{E_DEVICE, "internal: reprune of a unit whose build left a status word"};      // (the kernels have returned at once)
        u->stats.reprune_attempts = (uint32_t)attempt + 1;
        if (walk_ids_verdict(u, w)) { u->stats.device_bytes = u->arena.capacity(); continue; }
        break;
    }
    failed.armed = false;
    u->prm.coverage = coverage; u->downloaded = false;
    u->stats.ms_reprune = now_ms() - t0;
    trace(u, "reprune", t0, n_pos);
}

// the pinned buffers a download lands in (a one-shot unit: cut from its dead staged inputs)
void download_buffers(agx_unit *u) {
    const GraphCounts c = graph_counts(u);
    join_dl_helper(u);
    if (u->prm.flags & AGX_FLAG_ONE_SHOT) {
        // The inputs are in HBM and will not be uploaded again: their staged copies are dead pinned memory.  The download's arrays are cut
        // from the largest of those blocks, largest array first; what does not fit (thin read sets) gets a buffer of its own below.
        struct Room { char *at; size_t left; } room[LANDING_ROOMS]; int rooms = 0;
        landing_rooms(u, [&](auto &b, bool) { room[rooms++] = Room{(char *)b.p, b.block_bytes()}; });
        u->consumed = true; u->staged = false;
        size_t want[GA_N]; char *at[GA_N] = {};
        // (a loan from an earlier download of this unit object must not survive into alloc() below: the memory it names has been handed out again)
        graph_arrays(u, c, [&](int which, auto &h, auto &, size_t n, size_t pad) { h.release(); want[which] = ((n + pad) * sizeof(*h.p) + 255) & ~(size_t)255; });
        for (const int which : GRAPH_CUT_ORDER) for (Room &r : room) if (r.at && r.left >= want[which]) { at[which] = r.at; r.at += want[which]; r.left -= want[which]; break; }
        graph_arrays(u, c, [&](int which, auto &h, auto &, size_t n, size_t pad) { if (at[which]) h.borrow((decltype(h.p))at[which], n + pad); });
    }
    graph_arrays(u, c, [](int, auto &h, auto &, size_t n, size_t pad) { h.alloc(n + pad); });      // (keeps a loan, or a helper's buffer, that is large enough)
}

void do_download(agx_unit *u) {
    if (!u->built) do_build(u);
    HIP_OK(hipSetDevice(u->prm.device));             // the calling thread may never have touched this device
    const double t0 = now_ms();
    const GraphCounts c = graph_counts(u); const size_t n_pos = c.n_pos, ni = c.n_ids, ns = c.n_special;
    DeviceTurn &turn = turn_of(u->prm.device);
    download_buffers(u);
    u->dl_streaming = false;
    // the walk graph into the pinned buffers: plain copy commands on the device's download stream.  (r02 first used a kernel of its own for
    // this — copy commands seemed to queue behind other units' uploads; that was the hardware queue the streams shared.  Its stores to host
    // memory slowed whatever ran beside it, the next unit's binning most of all: the five builds of a cfg3 job ended at 45 ms with it, at
    // 42-45 ms with grids of 16-128 blocks, at 35 ms with the runtime's copies.)
    {
        void *dst[GA_N]; const void *src[GA_N]; size_t bytes[GA_N]; int n = 0;
        graph_arrays(u, c, [&](int, auto &h, auto &d, size_t count, size_t) { if (ni && count) { dst[n] = h.p; src[n] = d.p; bytes[n] = count * sizeof(*h.p); n++; } });      // (a unit without ids copies nothing, not even the one word its bitmap always has)
        bool by_engines = u->dl_sdma && n > 0;
        if (by_engines) {                            // (the build is complete and visible: this thread has waited for its last command)
            hsa_signal_store_relaxed(u->dl_signal, n);
            int queued = 0;
            for (; queued < n; queued++) if (hsa_amd_memory_async_copy(dst[queued], hsa_copy().cpu, src[queued], u->dl_agent, bytes[queued], 0, nullptr, u->dl_signal) != HSA_STATUS_SUCCESS) break;
            if (queued < n) hsa_signal_subtract_relaxed(u->dl_signal, n - queued);      // what was queued still counts down
            hsa_signal_value_t v;
            do v = hsa_signal_wait_scacquire(u->dl_signal, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED); while (v >= 1);      // (the wait may return early: only a value below 1 means the copies are done)
            if (queued < n || v < 0) { u->dl_sdma = false; by_engines = false; }        // the engines refused: this and every later download of the unit through HIP
        }
        if (!by_engines) {
            std::lock_guard<std::mutex> l(turn.down_m);
            for (int i = 0; i < n; i++) HIP_OK(hipMemcpyAsync(dst[i], src[i], bytes[i], hipMemcpyDeviceToHost, turn.down));
            HIP_OK(hipEventRecord(u->ev_dl, turn.down));
        }
    }
    const double t1 = now_ms();
    HIP_OK(wait_event(u->ev_dl));
    if (getenv("AGX_DL_TIMING")) fprintf(stderr, "[agx download] buffers %.2f ms, copies %.2f ms (%zu ids, %zu records)\n", t1 - t0, now_ms() - t1, ni, ns);
    memset(u->h_a_meta.p + ni, 0, 64);
    u->stats.n_walk_ids = ni; u->stats.n_special = ns;
    u->stats.download_bytes = graph_bytes(u, c);
    u->downloaded = true;
    u->stats.ms_download = now_ms() - t0;
    trace(u, u->dl_sdma ? "download (copy engines)" : "download (hipMemcpyAsync)", t0, n_pos);
}

// ---- streamed download (r06) ------------------------------------------------------------------------------------------------------------
// A unit's chain used to be upload -> build -> download -> walk in series; the walk of a large unit is split between walkers that each look at a WINDOW of the walk graph
// only (agx_walk.cpp: walk_split).  So the download goes out in position windows from the front — every window's meta bytes, bitmap words, ranks, records and hop entries of
// its main ids and of its positions' side ids; the bases last: the walk only takes byte ranges of them — each with its own completion signal, and agx_unit_finish starts
// the walk when the small head (side positions, overflow edges) is in.  A walker waits for its window (GraphView::wait_landed), the first walker — whose walks may lead anywhere
// — for all of them, and the stretches are cut by when the windows land.  What it takes off a unit's chain: about half its download (chr1 of configs[4]: 29 ms of 149).
// The cuts' ranks come with the build's counters (agx_cut_args).  Not for units that are trimmed after their download (agx_unit_download + agx_unit_trim: the caller wants the
// HBM back before the walk) — agx_unit_finish streams when nothing has been downloaded yet.
// (asleep: hsa_signal_wait spins whatever wait state it is asked for — sixteen walkers waiting for their windows burned 150 CPU-ms per cfg3 job — so: a short spin for what is about
// to land, then looks between short sleeps, like wait_event)
inline void wait_signal(hsa_signal_t g) {
    for (int i = 0; i < 64; i++) if (hsa_signal_load_scacquire(g) < 1) return;
    for (;;) { const timespec ts{0, 20000}; nanosleep(&ts, nullptr); if (hsa_signal_load_scacquire(g) < 1) return; }
}
std::atomic<double> &download_rate() { static std::atomic<double> r{40e6}; return r; }      // bytes per millisecond the engines have delivered (40 GB/s until measured)
void stream_wait_landed(void *ctx, agx_u32 main_hi, agx_u32 side_hi) {
    agx_unit *u = (agx_unit *)ctx; const int n = (int)u->cuts.n; int need = 0;
    while (need < n && (u->cut_main[need] < main_hi || u->cut_side[need] < side_hi)) need++;
    for (int p = 1; p <= need; p++) wait_signal(u->dl_piece[p]);
    if (need == n && !u->dl_timed.exchange(true)) {      // the last window is in: what the engines delivered per millisecond, for the next unit's estimate
        const double ms = now_ms() - u->dl_t0; u->stats.ms_download = ms;
        if (ms > 0.05 && u->dl_stream_bytes > (4u << 20)) download_rate().store(0.5 * download_rate().load() + 0.5 * std::min(std::max((double)u->dl_stream_bytes / ms, 35e6), 60e6));      // (clamped to what the link does: a download that queued behind another unit's, or whose last window was only looked at late, says little about it — chr1's 20 ms were once taken for 43)
        trace(u, "download (streamed): last window", u->dl_t0, u->V.n_pos);
    }
}
void stream_wait_str(void *ctx) { agx_unit *u = (agx_unit *)ctx; wait_signal(u->dl_piece[u->cuts.n + 1]); }
void stream_wait_all(agx_unit *u) { if (!u->dl_streaming) return; for (agx_u32 p = 0; p <= u->cuts.n + 1; p++) wait_signal(u->dl_piece[p]); u->dl_streaming = false; }

// false: this unit's download is not streamed (no cuts, no copy engines, counters that do not add up): the caller downloads the usual way
bool begin_streamed_download(agx_unit *u) {
    if (!u->built) do_build(u);
    const agx_u32 M = u->cuts.n;
    if (!M || !u->dl_sdma || getenv("AGX_NO_STREAM_DOWNLOAD")) return false;
    HIP_OK(hipSetDevice(u->prm.device));
    const double t0 = now_ms();
    const GraphCounts c = graph_counts(u); const size_t n_pos = c.n_pos, ni = c.n_ids, ns = c.n_special, nside = ni - n_pos;
    const agx_u32 *rank = u->h_words.p + W_CUT, *side = rank + (AGX_DL_PIECES + 1);
    // the cuts must be what the tables say: ranks and side counts ascending, every side id special, the last cut the whole table
    if (rank[0] != 0 || side[0] != 0 || side[M] != nside || (size_t)rank[M] + nside != ns) return false;
    for (agx_u32 w = 0; w < M; w++) if (rank[w] > rank[w + 1] || side[w] > side[w + 1]) return false;
    if (!u->dl_piece_made) { for (hsa_signal_t &g : u->dl_piece) if (hsa_signal_create(0, 0, nullptr, &g) != HSA_STATUS_SUCCESS) { u->dl_sdma = false; return false; } u->dl_piece_made = true; }
    download_buffers(u);
    memset(u->h_a_meta.p + ni, 0, 64);
    for (agx_u32 w = 0; w <= M; w++) { u->cut_main[w] = w == M ? (agx_u32)n_pos : u->cuts.word[w] * 64u; u->cut_side[w] = (agx_u32)n_pos + side[w]; }
    struct Copy { void *dst; const void *src; size_t bytes; int piece; };
    std::vector<Copy> copies; copies.reserve(12 * (size_t)M + 4);
    // the buffers, the sources, the counts and the element sizes are the declaration's (graph_arrays); which piece a range of an array travels in is decided here
    struct Arr { char *h; const char *d; size_t n, elem; } a[GA_N];
    graph_arrays(u, c, [&](int which, auto &h, auto &d, size_t n, size_t) { a[which] = Arr{(char *)h.p, (const char *)d.p, n, sizeof(*h.p)}; });
    auto add = [&](int piece, int which, size_t lo, size_t hi) { const Arr &x = a[which]; if (lo < hi) copies.push_back(Copy{x.h + lo * x.elem, x.d + lo * x.elem, (hi - lo) * x.elem, piece}); };
    add(0, GA_XPOS, 0, a[GA_XPOS].n); add(0, GA_OVF, 0, a[GA_OVF].n);
    add(0, GA_BITS, 0, a[GA_BITS].n); add(0, GA_RANK, 0, a[GA_RANK].n);      // (the bitmap and its ranks whole: 0.2 bytes per id, and two copies instead of four per window — a copy command costs the engines ~10 us)
    size_t main_bytes = 0;
    auto ids = [&](int piece, size_t lo, size_t hi, size_t r_lo, size_t r_hi) {      // everything about walk ids [lo, hi), whose records are [r_lo, r_hi) of the sparse table
        if (lo >= hi) return;
        add(piece, GA_META, lo, hi); add(piece, GA_NODE, r_lo, r_hi); add(piece, GA_HOP, r_lo, r_hi);
        main_bytes += (hi - lo) * a[GA_META].elem + (r_hi - r_lo) * (a[GA_NODE].elem + a[GA_HOP].elem);
    };
    for (agx_u32 w = 0; w < M; w++) {
        ids(1 + (int)w, u->cut_main[w], u->cut_main[w + 1], rank[w], rank[w + 1]);
        ids(1 + (int)w, u->cut_side[w], u->cut_side[w + 1], (size_t)rank[M] + side[w], (size_t)rank[M] + side[w + 1]);
    }
    add((int)M + 1, GA_STR, 0, a[GA_STR].n);      // the bases last: the walk only takes byte ranges of them
    int count[agx_unit::DL_SIGNALS] = {};
    for (const Copy &k : copies) count[k.piece]++;
    for (agx_u32 p = 0; p <= M + 1; p++) hsa_signal_store_relaxed(u->dl_piece[p], count[p]);
    u->dl_streaming = true; u->dl_timed.store(false); u->dl_t0 = now_ms(); u->dl_stream_bytes = main_bytes; u->dl_est_ms = (double)main_bytes / download_rate().load();
    size_t queued = 0;
    for (; queued < copies.size(); queued++) { const Copy &k = copies[queued]; if (hsa_amd_memory_async_copy(k.dst, hsa_copy().cpu, k.src, u->dl_agent, k.bytes, 0, nullptr, u->dl_piece[k.piece]) != HSA_STATUS_SUCCESS) break; }
    if (queued < copies.size()) {      // the engines refused: what was queued still counts down; then the usual way (through HIP from now on)
        for (size_t i = queued; i < copies.size(); i++) hsa_signal_subtract_relaxed(u->dl_piece[copies[i].piece], 1);
        stream_wait_all(u); u->dl_sdma = false; return false;
    }
    wait_signal(u->dl_piece[0]);
    u->stats.n_walk_ids = ni; u->stats.n_special = ns;
    u->stats.download_bytes = graph_bytes(u, c);
    trace(u, "download (streamed): queued, head in", t0, n_pos);
    return true;
}

// After the download: everything on the device that the walk cannot ask for (all but the arrays agx_walk_record reads, which lie at the front of the unit's block: pool_bufs)
// goes back to the device's memory region.  The unit is no longer built: another build uploads it again.  Returns the bytes given back (0: the block is not the region's — a
// unit below the region's threshold on a device without one —, or a capacity grew during the build and the arrays are no longer at the front).
size_t do_trim(agx_unit *u) {
    if (!u->downloaded) throw Error{E_ARG, "trim: the unit's walk graph has not been downloaded"};
    HIP_OK(hipSetDevice(u->prm.device));
    if (!u->arena.base()) return 0;
    // keep_end is where the kept front of the pool group ends in the arena's first block: as uploaded; or, after a pool regrow inside that block, the end of the new front (the old
    // one lies before it); or, after fetch_records regrew d_fetch inside it, the end of that.  ~0: the pool or d_fetch was regrown into a later block — nothing is given back.
    if (u->keep_end > u->arena.capacity()) return 0;
    const size_t freed = u->arena.shrink_to(u->keep_end);
    if (freed) { u->built = false; u->uploaded = false; }      // what lay behind the kept arrays is gone: the build's buffers, the uploaded inputs
    return freed;
}

// Gives back everything the unit holds on the device and its download buffers (to the caches of agx_mem.h: the next unit of the run takes
// them without a driver call).  The inputs stay staged: the unit can be uploaded again as if it were new.
void do_release(agx_unit *u) {
    const double tr0 = now_ms();
    if (u->pending_walk) { u->pending_walk = false; g_walks_pending.fetch_sub(1); }
    struct Tr { agx_unit *u; double t; ~Tr() { trace(u, "release", t, u->V.n_pos); } } tr{u, tr0};
    join_dl_helper(u);                                 // (it fills the download buffers released below)
    stream_wait_all(u);
    if (u->uploaded) { (void)hipSetDevice(u->prm.device); (void)hipEventSynchronize(u->ev_uploaded); (void)hipEventSynchronize(u->ev_built); (void)hipEventSynchronize(u->ev_dl); }      // (its commands are done before its memory goes)
    u->huge = false; u->dense = false;
    u->arena.reset();                                  // (empties every d_* view with it)
    graph_arrays(u, GraphCounts{}, [](int, auto &h, auto &, size_t, size_t) { h.release(); }); u->h_fetch.release();
    u->pool_cap = u->spill_lo = u->ovf_cap = u->list_cap = u->sp_cap = 0;
    u->uploaded = u->built = u->downloaded = false; u->support_valid = false;
    join_helper(u);
    u->out.pre_extended.clear(); u->out.extended.clear(); u->out_initial.clear(); u->out_ready = false;
    u->out.paths.clear(); u->out.paths_ready = false;
}

// records of non-special walk ids: built on the device from the node table, which stays in HBM (agx_walk_record), then one copy
void fetch_records(void *ctx, agx_u32 first, agx_u32 stride, agx_u32 rows, agx_u32 width, agx_walknode *out) {
    agx_unit *u = (agx_unit *)ctx;
    const size_t n = (size_t)rows * width;
    if (!n) return;
    if ((size_t)first + (size_t)(rows - 1) * stride + width > u->n_ids || n > 0x7FFFFFFFull) throw Error{E_ARG, "record fetch beyond the walk graph"};
    HIP_OK(hipSetDevice(u->prm.device));
    DeviceTurn &turn = turn_of(u->prm.device);
    std::lock_guard<std::mutex> l(turn.down_m);      // (also: the walkers of a large unit share the unit's fetch buffers)
    u->h_fetch.alloc(n);
    if (n > u->d_fetch.n) { u->d_fetch.alloc(u->arena, n); u->keep_end = u->arena.first_block_at(); }      // (it outlives the download: do_trim)
    agx_compact_args C = u->walk_args; C.n_ids = u->n_ids;
    agx_launch_fetch_records(&C, first, stride, rows, width, u->d_fetch.p, turn.down);
    HIP_OK(hipMemcpyAsync(u->h_fetch.p, u->d_fetch.p, n * sizeof(agx_walknode), hipMemcpyDeviceToHost, turn.down));
    HIP_OK(hipStreamSynchronize(turn.down));
    memcpy(out, u->h_fetch.p, n * sizeof(agx_walknode));
}

GraphView view_of(agx_unit *u) {
    GraphView G; G.n_pos = (agx_u32)u->V.n_pos; G.n_ids = u->n_ids;
    G.meta = u->h_a_meta.p; G.meta_rw = u->h_a_meta.p; G.str = u->h_a_str.p; G.side_xpos = u->h_side_xpos.p;
    G.sp_bits = u->h_sp_bits.p; G.sp_rank = u->h_sp_rank.p; G.sp_node = u->h_sp_node.p; G.sp_hop = u->h_sp_hop.p; G.n_special = u->n_special;
    G.fetch = fetch_records; G.fetch_ctx = u;
    G.ovf = u->h_a_ovf.p; G.n_ovf = u->n_ovf; G.row_slot = u->row_slot.empty() ? nullptr : u->row_slot.data();
    return G;
}


void write_file(const std::string &path, const std::string &data) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) throw Error{E_IO, "CANNOT OPEN FILE! (" + path + ")"};
    if (!data.empty() && fwrite(data.data(), 1, data.size(), f) != data.size()) { fclose(f); throw Error{E_IO, "short write to " + path}; }
    fclose(f);
}

}  // namespace

extern "C" {

const char *agx_version(void) { return "aligngraph_amd 0.1 (gfx950)"; }

int agx_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

int agx_selftest_scan(int device, uint32_t n, uint32_t seed) {
    try {
        HIP_OK(hipSetDevice(device));
        std::vector<agx_u32> in((size_t)n + 1, 0), want((size_t)n + 1), got((size_t)n + 1);
        agx_u32 x = seed * 2654435761u + 1u, acc = 0;
        for (uint32_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; in[i] = (x % 5u == 0) ? x % 97u : 0u; }       // mostly zeros, like the side-id counts
        for (uint32_t i = 0; i <= n; i++) { want[i] = acc; acc += in[i]; }
        const size_t nb = ((size_t)n + 1 + 4095) / 4096;
        DBuf<agx_u32> d_in, d_out; DBuf<unsigned long long> d_desc;
        DevArena arena; arena.device = device;
        d_in.alloc(arena, (size_t)n + 1); d_out.alloc(arena, (size_t)n + 1); d_desc.alloc(arena, nb + 1);
        HIP_OK(hipMemcpy(d_in.p, in.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_desc.p, 0, (nb + 1) * 8)); HIP_OK(hipMemset(d_out.p, 0xFF, ((size_t)n + 1) * 4));
        agx_launch_exclusive_scan1(d_in.p, d_out.p, n, d_desc.p, nullptr);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got.data(), d_out.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
        return got == want ? AGX_OK : AGX_E_DEVICE;
    } catch (const Error &) { return AGX_E_DEVICE; }
}

// ---- test hooks of the primitives under every build and export (tests/test_gpu_primitives.py): the caller's arrays through the product's launchers, every device array
// followed (agx_test_zero: also preceded) by AGX_TEST_GUARD words of 0xA5 bytes that come back with it.  They need no unit, and a build that does not call them runs none of this.
int agx_test_scan(int device, int form, const uint32_t *in, uint32_t n, uint32_t *out, uint32_t grid_cap, int seeded, int streams, uint64_t *desc, uint32_t *tmp, uint32_t *grid_limit) {
    if (!in || !out || (form != 0 && form != 1) || n == 0xFFFFFFFFu || streams < 1 || streams > 2 || (streams == 2 && grid_cap)) return AGX_E_ARG;
    if (form == 0 ? (!tmp || grid_cap || seeded) : !desc) return AGX_E_ARG;
    hipStream_t st[2] = {nullptr, nullptr};
    int rc = AGX_OK;
    try {
        HIP_OK(hipSetDevice(device));
        const size_t m = (size_t)n + 1, G = AGX_TEST_GUARD, nb = (m + 4095) / 4096, nb2 = (nb + 4095) / 4096, tw = 2 * (nb + 1) + 2 * (nb2 + 1);
        DBuf<agx_u32> d_in, d_out[2], d_tmp[2]; DBuf<unsigned long long> d_desc[2];
        DevArena arena; arena.device = device;
        std::vector<unsigned long long> d0(nb + G, 0xA5A5A5A5A5A5A5A5ull);      // the descriptors as the launch finds them: zero, or (seeded) every block's own aggregate already there
        for (size_t b = 0; b < nb; b++) {
            agx_u32 t = 0;
            if (seeded) for (size_t i = b * 4096; i < m && i < (b + 1) * 4096; i++) t += in[i];
            d0[b] = seeded ? AGX_SCAN_AGG | t : 0ull;
        }
        d_in.alloc(arena, m);
        HIP_OK(hipMemcpy(d_in.p, in, m * 4, hipMemcpyHostToDevice));
        for (int s = 0; s < streams; s++) {
            d_out[s].alloc(arena, m + G); HIP_OK(hipMemset(d_out[s].p, 0xA5, (m + G) * 4));
            if (form == 1) { d_desc[s].alloc(arena, nb + G); HIP_OK(hipMemcpy(d_desc[s].p, d0.data(), (nb + G) * 8, hipMemcpyHostToDevice)); }
            else { d_tmp[s].alloc(arena, tw + G); HIP_OK(hipMemset(d_tmp[s].p, 0xA5, (tw + G) * 4)); }
        }
        if (streams == 2) for (int s = 0; s < 2; s++) HIP_OK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));      // (a build's front and main stream)
        HIP_OK(hipDeviceSynchronize());
        if (grid_limit) *grid_limit = agx_scan_grid_limit(grid_cap);
        for (int s = 0; s < streams; s++) {
            if (form == 1) agx_launch_exclusive_scan1_capped(d_in.p, d_out[s].p, n, d_desc[s].p, grid_cap, st[s]);
            else agx_launch_exclusive_scan(d_in.p, d_out[s].p, n, d_tmp[s].p, st[s]);
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        for (int s = 0; s < streams; s++) {
            HIP_OK(hipMemcpy(out + (size_t)s * (m + G), d_out[s].p, (m + G) * 4, hipMemcpyDeviceToHost));
            if (form == 1) HIP_OK(hipMemcpy(desc + (size_t)s * (nb + G), d_desc[s].p, (nb + G) * 8, hipMemcpyDeviceToHost));
            else HIP_OK(hipMemcpy(tmp + (size_t)s * (tw + G), d_tmp[s].p, (tw + G) * 4, hipMemcpyDeviceToHost));
        }
    } catch (const Error &) { rc = AGX_E_DEVICE; }
      catch (const std::bad_alloc &) { rc = AGX_E_ARG; }
    for (hipStream_t s : st) if (s) (void)hipStreamDestroy(s);
    return rc;
}

int agx_test_zero(int device, const uint32_t *len, uint32_t *words) {
    if (!len || !words) return AGX_E_ARG;
    try {
        HIP_OK(hipSetDevice(device));
        const size_t G = AGX_TEST_GUARD;
        DBuf<agx_u32> d[8];
        DevArena arena; arena.device = device;
        agx_zero_args Z; memset(&Z, 0, sizeof Z);
        for (int s = 0; s < 8; s++) {
            d[s].alloc(arena, (size_t)len[s] + 2 * G); HIP_OK(hipMemset(d[s].p, 0xA5, ((size_t)len[s] + 2 * G) * 4));
            Z.p[s] = d[s].p + G; Z.n[s] = len[s];
        }
        HIP_OK(hipDeviceSynchronize());
        agx_launch_zero(&Z, nullptr);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        size_t at = 0;
        for (int s = 0; s < 8; s++) { HIP_OK(hipMemcpy(words + at, d[s].p, ((size_t)len[s] + 2 * G) * 4, hipMemcpyDeviceToHost)); at += (size_t)len[s] + 2 * G; }
        return AGX_OK;
    } catch (const Error &) { return AGX_E_DEVICE; }
      catch (const std::bad_alloc &) { return AGX_E_ARG; }
}

int agx_test_copy_out(int device, int n_seg, const uint64_t *bytes, const uint8_t *src, uint8_t *dst) {
    if (n_seg < 1 || n_seg > 16 || !bytes || !src || !dst) return AGX_E_ARG;
    try {
        HIP_OK(hipSetDevice(device));
        const size_t G = AGX_TEST_GUARD * 4;
        DBuf<agx_u8> d_src[16]; PBuf<agx_u8> h_dst;
        DevArena arena; arena.device = device;
        size_t total = 0, at = 0, from = 0;
        for (int s = 0; s < n_seg; s++) total += ((size_t)bytes[s] + 15) / 16 * 16 + G;
        h_dst.alloc(total); memset(h_dst.p, 0xA5, total);
        void *dp[16]; const void *sp[16]; size_t nbytes[16];
        for (int s = 0; s < n_seg; s++) {
            const size_t r = ((size_t)bytes[s] + 15) / 16 * 16;
            d_src[s].alloc(arena, r);
            if (r) HIP_OK(hipMemcpy(d_src[s].p, src + from, r, hipMemcpyHostToDevice));
            dp[s] = (char *)h_dst.dev() + at; sp[s] = d_src[s].p; nbytes[s] = (size_t)bytes[s];
            at += r + G; from += r;
        }
        HIP_OK(hipDeviceSynchronize());
        agx_launch_copy_out(dp, sp, nbytes, n_seg, nullptr);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        memcpy(dst, h_dst.p, total);
        return AGX_OK;
    } catch (const Error &) { return AGX_E_DEVICE; }
      catch (const std::bad_alloc &) { return AGX_E_ARG; }
}

int agx_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
    size_t f = 0, t = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess) return AGX_E_DEVICE;
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return AGX_OK;
}

int agx_unit_create(const agx_params *p, agx_unit **out) {
    if (!p || !out) return AGX_E_ARG;
    *out = nullptr;
    if (p->k == 0 || p->k >= 32768) return AGX_E_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return AGX_E_NOGPU;
    if (p->device < 0 || p->device >= n) return AGX_E_ARG;
    agx_unit *u = new (std::nothrow) agx_unit();
    if (!u) return AGX_E_ARG;
    u->prm = *p; if (u->prm.batch == 0) u->prm.batch = 1000000;
    const int rc = guarded(u, [&] {
        try { u->helper.start(); } catch (...) { }      // (without it the unit prepares its buffers on the caller's threads)
        HIP_OK(hipSetDevice(p->device));
        u->ev.init(); u->ev.all = (u->prm.flags & AGX_FLAG_TIME_SECTIONS) != 0;
        for (hipEvent_t *e : {&u->ev_front, &u->ev_passA, &u->ev_passJ}) HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        for (hipEvent_t *e : {&u->ev_dl, &u->ev_built, &u->ev_hits}) HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        HIP_OK(hipEventCreate(&u->ev_up0)); HIP_OK(hipEventCreate(&u->ev_uploaded));
        for (int i = 0; i < 8; i++) { HIP_OK(hipEventCreateWithFlags(&u->ev_rows[i], hipEventDisableTiming)); HIP_OK(hipEventCreateWithFlags(&u->ev_win[i], hipEventDisableTiming)); HIP_OK(hipEventCreate(&u->ev_sw0[i])); HIP_OK(hipEventCreate(&u->ev_sw1[i])); }
        u->dl_sdma = hsa_copy().agent_of(p->device, u->dl_agent) && hsa_signal_create(0, 0, nullptr, &u->dl_signal) == HSA_STATUS_SUCCESS;
    });
    if (rc != AGX_OK) { delete u; return rc; }
    g_units_alive.fetch_add(1);
    *out = u;
    return AGX_OK;
}

void agx_unit_destroy(agx_unit *u) { if (u) { (void)hipSetDevice(u->prm.device); do_release(u); delete u; if (g_units_alive.fetch_sub(1) == 1) out_cache_trim(); } }

const char *agx_unit_error(const agx_unit *u) { return u ? u->err.c_str() : "null unit"; }

int agx_unit_set_reference(agx_unit *u, const char *bases, uint32_t n) {
    if (!u || (!bases && n)) return AGX_E_ARG;
    return guarded(u, [&] { drop_outputs(u); u->T = Threads(); u->T.ref.assign(bases, n); u->T.n_ref = n; u->have_ref = true; u->have_threads = false; u->staged = false; u->uploaded = false; u->built = false; });
}

int agx_unit_set_contig_threads(agx_unit *u, const char *appended, uint32_t n_appended, const uint32_t *cm_start, const agx_contimer *cm, uint32_t n_cm,
                                const char *initial_contigs, size_t initial_len) {
    if (!u || !cm_start || (!cm && n_cm) || (!appended && n_appended)) return AGX_E_ARG;
    return guarded(u, [&] {
        if (!u->have_ref) throw Error{E_ARG, "set the reference first"};
        drop_outputs(u);
        u->T.ref.resize(u->T.n_ref); u->T.ref.append(appended ? appended : "", n_appended);
        const size_t n_pos = u->T.ref.size();
        u->T.cm_start.assign(cm_start, cm_start + n_pos + 1);
        if (u->T.cm_start[n_pos] != n_cm) throw Error{E_ARG, "cm_start does not end at n_cm"};
        u->T.cm.resize(n_cm);
        for (uint32_t i = 0; i < n_cm; i++) {
            if (cm[i].next_off != AGX_NONE && cm[i].next_off >= n_pos) throw Error{E_ARG, "conti-mer link beyond the position array"};
            u->T.cm[i] = ContiMer{cm[i].nuc, cm[i].cid, cm[i].coff, cm[i].next_off, cm[i].next_item};
        }
        u->T.initial_contigs.assign(initial_contigs ? initial_contigs : "", initial_len);
        build_chains(u->T);
        u->have_threads = true; u->staged = false; u->uploaded = false; u->built = false;
    });
}

int agx_unit_push_pairs(agx_unit *u, const agx_pair_batch *b) {
    if (!u || !b) return AGX_E_ARG;
    return guarded(u, [&] {
        drop_outputs(u);
        if (u->pairs_staged) { u->pairs_staged = false; u->row_off.clear(); u->reads_keep.reset(); u->P = Pairs(); }
        if (u->P.hits.empty()) { u->P = Pairs(); u->P.stride = b->stride; }
        if (b->stride != u->P.stride) throw Error{E_ARG, "all batches of a unit must use one read stride"};
        const agx_u32 slot0 = u->P.n_slots, run0 = (agx_u32)u->P.runs.size();
        for (uint64_t i = 0; i < b->n_hits; i++) {
            agx_hit h = b->hits[i];
            if (h.len == 0 || h.len > b->stride || (uint64_t)h.slot1 + 1 >= b->n_slots) throw Error{E_ARG, "hit names a read slot outside the batch"};
            if ((h.nruns1 && (uint64_t)h.runs1 + h.nruns1 > b->n_runs) || (h.nruns2 && (uint64_t)h.runs2 + h.nruns2 > b->n_runs)) throw Error{E_ARG, "hit names runs outside the batch"};
            if (h.back > i) throw Error{E_ARG, "hit.back reaches before the batch"};
            h.slot1 += slot0; if (h.nruns1) h.runs1 += run0; if (h.nruns2) h.runs2 += run0;
            u->P.hits.push_back(h);
        }
        u->P.runs.insert(u->P.runs.end(), b->runs, b->runs + b->n_runs);
        u->P.bases.append(b->bases, (size_t)b->n_slots * b->stride);
        u->P.n_slots += b->n_slots;
        u->staged = false; u->uploaded = false; u->built = false;
    });
}

struct agx_reads { std::shared_ptr<agx::ReadsIndex> idx; };

int agx_reads_open(const char *reads_fa, agx_reads **out, char *err, size_t err_len) {
    if (!reads_fa || !out) return AGX_E_ARG;
    *out = nullptr;
    try { std::unique_ptr<agx_reads> r(new agx_reads); r->idx.reset(reads_index_open(reads_fa), reads_index_close); *out = r.release(); return AGX_OK; }
    catch (const Error &e) { if (err && err_len) snprintf(err, err_len, "%s", e.msg.c_str()); return e.code ? e.code : AGX_E_ARG; }
    catch (const std::exception &e) { if (err && err_len) snprintf(err, err_len, "%s", e.what()); return AGX_E_ARG; }
}

void agx_reads_close(agx_reads *reads) { delete reads; }      // (units that were loaded through it keep the mapping alive for as long as they need it)

int agx_unit_load_files(agx_unit *u, const char *tmp_dir, int unit) { return agx_unit_load_files_shared(u, tmp_dir, unit, nullptr); }

// The five text files of a unit -> staged arrays.  Three independent pieces of work — the unit sequence + contig threading, the read alignments, and
// (without a shared agx_reads) the index of tmp/_reads.fa — of which the first runs on a thread of its own beside the others.  Each piece first
// tries the fast loader (agx_load.cpp) and takes the general one (agx_host.cpp) when that declines; AGX_NO_FAST_LOAD=1 turns the fast ones off.
int agx_unit_load_files_shared(agx_unit *u, const char *tmp_dir, int unit, const agx_reads *reads) {
    if (!u || !tmp_dir) return AGX_E_ARG;
    return guarded(u, [&] {
        const std::string d = tmp_dir, s = std::to_string(unit);
        u->stats.from_cache = 0;
        u->choice = upload_choice();                      // (the loaders' buffers and the cache's staging follow it)
        if (load_cache(u, d, unit)) return;              // the unit's staged form, written when the alignments were distributed (agx_unit_cache_build)
        const double t0 = now_ms();
        const bool fast = getenv("AGX_NO_FAST_LOAD") == nullptr;
        drop_outputs(u);
        HIP_OK(hipSetDevice(u->prm.device));              // (the fast loader writes into pinned memory, and registering it needs a current device)
        u->T = Threads(); u->P = Pairs(); u->pairs_staged = false; u->row_off.clear(); u->row_slot.clear(); u->reads_keep.reset(); u->reads_map.reset(); u->cache_map.reset(); u->pairs_file = agx::PairsFile();
        u->staged = false; u->uploaded = false; u->built = false; u->consumed = false;      // (new inputs: whatever a download did to the old staged ones no longer matters)
        double ms_thread = 0;
        std::exception_ptr thread_err;
        auto threads_job = [&] {
            try {
                const double a = now_ms();
                load_unit_reference(d + "/_genome." + s + ".fa", u->T.ref);
                if (!(fast && thread_contigs_fast(d + "/_contigs.fa", d + "/_contigs_genome." + s + ".psl", u->T)))
                    thread_contigs_from_files(d + "/_contigs.fa", d + "/_contigs_genome." + s + ".psl", u->T);
                ms_thread = now_ms() - a;
            } catch (...) { thread_err = std::current_exception(); }
        };
        std::thread side; bool side_started = false;
        try { side = std::thread(threads_job); side_started = true; } catch (const std::system_error &) { }
        struct Join { std::thread &t; bool on; ~Join() { if (on && t.joinable()) t.join(); } } join{side, side_started};
        if (!side_started) threads_job();
        if (thread_err && !side_started) std::rethrow_exception(thread_err);      // (the reference loads the genome and the contig alignment first: their errors come first)
        const double tp0 = now_ms();
        std::exception_ptr pairs_err;
        try {
            const std::string sam = d + "/_reads_genome." + s + ".bowtie";
            bool done = false;
            {   // the alignments handed over staged (tmp/_agx_pairs.<u>.bin) stand in for the two text files
                agx::PairsFile F;
                if (open_pairs_file(pairsfile::path_of(d, unit), F)) { load_staged_pairs(u, F); done = true; }
            }
            std::shared_ptr<ReadsIndex> idx = done ? std::shared_ptr<ReadsIndex>() : reads ? reads->idx : std::shared_ptr<ReadsIndex>(reads_index_open(d + "/_reads.fa"), reads_index_close);
            if (!done && fast) {
                struct stat sb; const size_t sam_bytes = stat(sam.c_str(), &sb) == 0 ? (size_t)sb.st_size : 0;
                UnitSink sink(u); StagedPairs S;
                if (load_pairs_fast(*idx, sam, (long)u->prm.batch, u->prm.k, loader_threads(sam_bytes), sink, S)) { adopt_pairs(u, S); u->pairs_staged = true; u->reads_keep = idx; u->n_slots = 0; done = true; }
            }
            if (!done) load_pairs_from_files(d + "/_reads.fa", sam, (long)u->prm.batch, u->prm.k, u->P, idx.get());
        } catch (...) { pairs_err = std::current_exception(); }
        if (side_started) { side.join(); join.on = false; }
        if (thread_err) std::rethrow_exception(thread_err);
        if (pairs_err) std::rethrow_exception(pairs_err);
        if (u->pairs_staged && u->pairs_file.fv)      // the rules of the staged-pairs file that need the unit's positions, now that the threading has said how many there are
            if (const char *rule = staged_positions_rule(staged_view(u, u->n_rows, u->stride, u->maxlen, u->T.ref.size()), std::min(8u, std::max(1u, usable_cpus())))) {
                u->pairs_staged = false; u->pairs_file = agx::PairsFile(); u->have_ref = u->have_threads = false;      // (nothing of the file stays with the unit)
                throw Error{E_FORMAT, std::string("tmp/_agx_pairs: the staged arrays are inconsistent (") + rule + ")"};
            }
        u->stats.ms_thread = ms_thread; u->stats.ms_parse = now_ms() - tp0;
        u->have_ref = u->have_threads = true;
        stage_inputs(u);
        u->stats.ms_stage = now_ms() - t0 - u->stats.ms_parse;      // (what the load took beyond the read alignments: staging, and whatever of the contig threading was not hidden behind them)
    });
}

int agx_unit_cache_build(const agx_params *p, const char *tmp_dir, int unit, const agx_reads *reads, char *err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    if (!p || !tmp_dir) return AGX_E_ARG;
    agx_unit *u = nullptr;
    agx_params once; if (p) { once = *p; once.flags |= AGX_FLAG_ONE_SHOT; }      // loaded, built and thrown away here
    int rc = agx_unit_create(p ? &once : nullptr, &u);
    if (rc != AGX_OK) { if (err && err_len) snprintf(err, err_len, "%s", rc == AGX_E_NOGPU ? "no HIP device" : "bad parameters"); return rc; }
    rc = agx_unit_load_files_shared(u, tmp_dir, unit, reads);      // (takes a current cache file if there is one)
    if (rc == AGX_OK && !u->stats.from_cache) rc = guarded(u, [&] { save_cache(u, tmp_dir, unit); });
    if (rc != AGX_OK && err && err_len) snprintf(err, err_len, "%s", agx_unit_error(u));
    agx_unit_destroy(u);
    return rc;
}

int agx_unit_cache_save(agx_unit *u, const char *tmp_dir, int unit) { if (!u || !tmp_dir) return AGX_E_ARG; return guarded(u, [&] { save_cache(u, tmp_dir, unit); }); }

int agx_unit_hbm_needed(agx_unit *u, uint64_t *bytes) {
    if (!u || !bytes) return AGX_E_ARG;
    return guarded(u, [&] { if (!u->staged) stage_inputs(u); *bytes = round_block(plan_capacities(u).total); });
}

int agx_unit_stage(agx_unit *u) { if (!u) return AGX_E_ARG; return guarded(u, [&] { stage_inputs(u); }); }
int agx_unit_upload(agx_unit *u) { if (!u) return AGX_E_ARG; return guarded(u, [&] { do_upload(u); }); }
int agx_unit_release(agx_unit *u) { if (!u) return AGX_E_ARG; return guarded(u, [&] { do_release(u); }); }
int agx_unit_trim(agx_unit *u, uint64_t *freed) { if (!u) return AGX_E_ARG; if (freed) *freed = 0; return guarded(u, [&] { const size_t f = do_trim(u); u->trimmed = true; if (freed) *freed = f; }); }
void agx_pool_trim(int device) { if (device >= 0) dev_trim(device); else if (device == -1) { host_trim(); scratch_trim(); out_cache_trim(); } else host_retire(); }      // (-1 also unmaps the loaders' cached scratch memory: up to 16 GB of touched pages per process otherwise stay until exit)
int agx_unit_build(agx_unit *u) { if (!u) return AGX_E_ARG; return guarded(u, [&] { do_build(u); }); }
int agx_unit_reprune(agx_unit *u, uint32_t coverage) { if (!u) return AGX_E_ARG; return guarded(u, [&] { do_reprune(u, coverage); }); }
int agx_unit_download(agx_unit *u) { if (!u) return AGX_E_ARG; return guarded(u, [&] { do_download(u); }); }

int agx_unit_finish(agx_unit *u, agx_result *r) {
    if (!u || !r) return AGX_E_ARG;
    memset(r, 0, sizeof *r);
    return guarded(u, [&] {
        // nothing downloaded yet: the download is streamed where it can be, and the walk begins on what has landed (begin_streamed_download)
        const bool streamed = !u->downloaded && begin_streamed_download(u);
        if (!u->downloaded && !streamed) do_download(u);
        struct Landed { agx_unit *u; ~Landed() { stream_wait_all(u); } } landed{u};      // (also if the walk throws: the copies write into buffers that are released afterwards)
        const double t0 = now_ms();
        join_helper(u);
        prepare_outputs(u);               // (a unit whose helper could not make them, or that is finished a second time)
        if (!u->out_ready) throw Error{E_ARG, "out of host memory"};
        u->downloaded = false;            // the walk marks the downloaded meta bytes: another finish downloads again
        u->out_ready = false;             // (an error below leaves the buffers to the next prepare_outputs)
        // Walkers for this walk: sixteen while few units are on the way (five at most) and at most two other walks are running, or nobody else is on the way — a job's tail: the
        // walkers of two or three walks on 16 CPUs fill each other's waits (cfg3: 33.2 -> 32.2 ms per job at +15 % CPU time); else eight, or what the walker threads already
        // running leave of this process's CPUs: a job with eight units in flight is bound by its CPU time (the whole-human job: 572 ms with this rule, 589 ms with sixteen walkers
        // whenever two walks or fewer were running).
        // (r04 gave sixteen to the last walk only; since r05 a job's builds end closer together than its walks take.)
        static std::atomic<int> walkers_busy{0}, walks_running{0};
        {   static const int ranks = [] { const char *e = getenv("LOCAL_WORLD_SIZE"); const int n = e ? atoi(e) : 1; return n < 1 ? 1 : n; }();
            const int free_cpus = (int)usable_cpus() / ranks - walkers_busy.load();
            agx::walkers_cap = (g_walks_pending.load() <= 1 || (g_walks_pending.load() <= 5 && walks_running.load() <= 2)) ? (int)GraphView::MAX_WALKERS : std::max(8, std::min((int)GraphView::MAX_WALKERS, free_cpus)); }
        struct Busy { std::atomic<int> &n, &w; int k; Busy(std::atomic<int> &c, std::atomic<int> &r, int walkers) : n(c), w(r), k(walkers) { n.fetch_add(k); w.fetch_add(1); } ~Busy() { n.fetch_sub(k); w.fetch_sub(1); } } busy{walkers_busy, walks_running, walkers_now(u->V.n_pos)};
        struct Walked { agx_unit *u; ~Walked() { if (u->pending_walk) { u->pending_walk = false; g_walks_pending.fetch_sub(1); } } } walked{u};
        struct Helpers : Assistant {           // helper 0: the unit's own thread (formats the written records while the walk goes on, or walks a stretch); 1..: pool threads for further walkers
            agx_unit *u; int pool[GraphView::MAX_WALKERS] = {}; int n_pool = 0;
            Helpers(agx_unit *x, int extra) : u(x) { for (int i = 0; i < extra && i < GraphView::MAX_WALKERS - 2; i++) { const int t = walker_pool().take(); if (t < 0) break; pool[n_pool++] = t; } }
            ~Helpers() override { for (int i = 0; i < n_pool; i++) { walker_pool().wait(pool[i]); walker_pool().give(pool[i]); } }
            int helpers() const override { return 1 + n_pool; }
            void run(std::function<void()> f, int who) override {
                if (who == 0) { if (!u->helper.submit(UnitHelper::WALK, std::move(f))) throw Error{E_ARG, "no helper thread"}; }
                else walker_pool().run(pool[who - 1], std::move(f));
            }
            void wait(int who) override { if (who == 0) u->helper.wait(UnitHelper::WALK); else walker_pool().wait(pool[who - 1]); }
        } second(u, walkers_now(u->V.n_pos) - 2);      // one thread per further walker: the unit's helper + pool threads
        GraphView G = view_of(u);
        if (streamed) { G.wait_landed = stream_wait_landed; G.wait_str = stream_wait_str; G.land_ctx = u; G.land_ms = std::max(0.01, u->dl_est_ms - (now_ms() - u->dl_t0)); }
        u->out.keep_paths = (u->prm.flags & AGX_FLAG_KEEP_PATHS) != 0; u->out.paths.clear(); u->out.paths_ready = false;
        walk_join_scaffold(u->V, G, u->out, u->helper.started ? &second : nullptr);
        u->out.paths_ready = u->out.keep_paths;
        u->stats.ms_walk = now_ms() - t0; u->stats.n_fetched = u->out.n_fetched;
        trace(u, "walk", t0, u->V.n_pos);
        r->initial_len = u->out_initial.n; r->initial_contigs = u->out_initial.release();
        r->pre_len = u->out.pre_extended.n; r->pre_extended = u->out.pre_extended.release();
        r->extended_len = u->out.extended.n; r->extended = u->out.extended.release();
    });
}

void agx_result_free(agx_result *r) { if (!r) return; out_cache_give(r->initial_contigs); out_cache_give(r->pre_extended); out_cache_give(r->extended); memset(r, 0, sizeof *r); }      // (kept for the next unit's outputs: agx_host.h)

int agx_unit_stats(const agx_unit *u, agx_stats *s) {
    if (!u || !s) return AGX_E_ARG;
    *s = u->stats;
    const bool st = u->staged || u->consumed;      // (a one-shot unit's staged inputs are gone after its download; their counts are not)
    s->n_pos = st ? u->V.n_pos : u->T.ref.size(); s->n_ref = st ? u->V.n_ref : u->T.n_ref; s->n_hits = st ? u->nh : u->P.hits.size(); s->n_runs = st ? u->n_runs : u->P.runs.size(); s->pinned_bytes_cached = host_cache().held(); s->device_bytes_cached = dev_cache(u->prm.device).held(); s->n_nodes = u->n_nodes;
    s->n_tiles = u->n_tiles; s->n_tile_entries = u->n_tile_entries; s->n_big_tiles = u->n_big; s->n_mid_tiles = u->n_mid; s->n_edge_overflow = u->n_ovf; s->n_edge_slow = u->n_slow;
    s->pairs_in_file = u->pairs_in_file; s->sam_line_pairs = u->sam_pairs;
    return AGX_OK;
}

// canonical numbering (position-major, variant order) of the used slots of a node table that came down whole: canon[slot] = id (NONE: unused), slot_of[id] = slot
extern "C++" void agx::number_nodes(const std::vector<agx_u32> &node_start, const std::vector<agx_u16> &node_cnt, agx_u32 cap, agx_u32 nn, std::vector<agx_u32> &canon, std::vector<agx_u32> &slot_of, uint32_t *start_out) {
    canon.assign(cap, AGX_NONE); slot_of.assign(nn, 0); agx_u32 id = 0;
    const agx_u32 n_pos = (agx_u32)node_start.size();
    for (agx_u32 x = 0; x < n_pos; x++) {
        if (start_out) start_out[x] = id;
        for (agx_u32 v = 0; v < node_cnt[x]; v++) {
            if ((size_t)node_start[x] + v >= cap || id >= nn) throw Error{E_DEVICE, "node table is inconsistent (count mismatch)"};
            slot_of[id] = node_start[x] + v; canon[node_start[x] + v] = id++;
        }
    }
    if (start_out) start_out[n_pos] = id;
    if (id != nn) throw Error{E_DEVICE, "node table is inconsistent (count mismatch)"};
}

int agx_unit_graph(agx_unit *u, agx_graph *g) {
    if (!u || !g) return AGX_E_ARG;
    memset(g, 0, sizeof *g);
    return guarded(u, [&] {
        if (!u->built) do_build(u);
        HIP_OK(hipSetDevice(u->prm.device));
        HIP_OK(wait_event(u->ev_built));
        // the pool has unused slots (one slice per region): the arrays come down whole, nodes are reached through node_start / node_cnt
        const agx_u32 n_pos = (agx_u32)u->V.n_pos, nn = u->n_nodes, cap = u->pool_cap;
        std::vector<agx_u32> node_start(n_pos), cid(cap), coff(cap), cid0(cap), coff0(cap), off0(cap), next((size_t)cap * AGX_MAXE); std::vector<agx_u16> node_cnt(n_pos);
        std::vector<agx_sref> sref(cap); std::vector<int> counts; std::vector<agx_edge_ovf> ovf(u->n_ovf);
        HIP_OK(hipMemcpy(node_start.data(), u->d_node_start.p, (size_t)n_pos * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(node_cnt.data(), u->d_node_cnt.p, (size_t)n_pos * 2, hipMemcpyDeviceToHost));
        if (cap) {
            HIP_OK(hipMemcpy(cid.data(), u->d_cid.p, (size_t)cap * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(coff.data(), u->d_coff.p, (size_t)cap * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(cid0.data(), u->d_cid0.p, (size_t)cap * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(coff0.data(), u->d_coff0.p, (size_t)cap * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(off0.data(), u->d_off0.p, (size_t)cap * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(next.data(), u->d_next.p, (size_t)cap * AGX_MAXE * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(sref.data(), u->d_sref.p, (size_t)cap * sizeof(agx_sref), hipMemcpyDeviceToHost));
            if (u->prm.flags & AGX_FLAG_KEEP_COUNTS) { counts.resize((size_t)cap * 6); HIP_OK(hipMemcpy(counts.data(), u->d_counts.p, (size_t)cap * 24, hipMemcpyDeviceToHost)); }
        }
        if (u->n_ovf) HIP_OK(hipMemcpy(ovf.data(), u->d_ovf.p, (size_t)u->n_ovf * sizeof(agx_edge_ovf), hipMemcpyDeviceToHost));
        g->n_pos = n_pos; g->n_nodes = nn;
        g->node_start = (uint32_t *)malloc(4 * ((size_t)n_pos + 1)); g->node_key = (uint32_t *)malloc(24 * ((size_t)nn + 1)); g->node_cnt = (int32_t *)malloc(24 * ((size_t)nn + 1));
        g->node_slen = (uint32_t *)malloc(4 * ((size_t)nn + 1)); g->edge_start = (uint32_t *)malloc(4 * ((size_t)nn + 1));
        std::vector<agx_u32> canon, slot_of;
        number_nodes(node_start, node_cnt, cap, nn, canon, slot_of, g->node_start);
        std::vector<std::vector<agx_u32> > adj(nn);
        for (agx_u32 c = 0; c < nn; c++) for (agx_u32 e = 0; e < AGX_MAXE; e++) { const agx_u32 d = next[(size_t)slot_of[c] * AGX_MAXE + e]; if (d != AGX_NONE) adj[c].push_back(canon[d]); }
        for (agx_u32 i = 0; i < u->n_ovf; i++) adj[canon[ovf[i].src]].push_back(canon[ovf[i].dst]);
        size_t ne = 0;
        for (auto &a : adj) { std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end()); ne += a.size(); }
        g->n_edges = (uint32_t)ne; g->edge_dst = (uint32_t *)malloc(4 * (ne + 1));
        for (agx_u32 c = 0; c < nn; c++) {
            const agx_u32 v = slot_of[c]; uint32_t *kk = g->node_key + 6 * (size_t)c;
            kk[0] = cid[v]; kk[1] = coff[v]; kk[2] = cid0[v]; kk[3] = coff0[v]; kk[4] = off0[v] == AGX_NONE ? AGX_NONE : 0; kk[5] = off0[v];
            if (!counts.empty()) memcpy(g->node_cnt + 6 * (size_t)c, counts.data() + 6 * (size_t)v, 24); else for (int j = 0; j < 6; j++) g->node_cnt[6 * (size_t)c + j] = -1;
            g->node_slen[c] = (sref[v].qlen >> 16) & 0x7FFF;
        }
        size_t eo = 0;
        for (agx_u32 c = 0; c < nn; c++) { g->edge_start[c] = (uint32_t)eo; for (agx_u32 d : adj[c]) g->edge_dst[eo++] = d; }
        g->edge_start[nn] = (uint32_t)eo;
    });
}

void agx_graph_free(agx_graph *g) {
    if (!g) return;
    free(g->node_start); free(g->node_key); free(g->node_cnt); free(g->node_slen); free(g->edge_start); free(g->edge_dst); memset(g, 0, sizeof *g);
}

// Test and inspection hook: the walk graph exactly as view_of() hands it to the walk, copied out before any walk has marked a_meta.
int agx_unit_walk_graph(agx_unit *u, int streamed, agx_walk_graph *g) {
    if (!u || !g) return AGX_E_ARG;
    const bool want_all = g->want_all_node != 0;
    memset(g, 0, sizeof *g);
    const int rc = guarded(u, [&] {
        static_assert(sizeof(agx_walk_rec) == sizeof(agx_walknode) && sizeof(agx_walk_hop) == sizeof(agx_hop), "include/agx.h mirrors the walk graph's records");
        if (u->prm.flags & AGX_FLAG_ONE_SHOT) throw Error{E_ARG, "walk graph: a one-shot unit's download lands in its staged inputs and cannot be repeated for the walk"};
        if (streamed) {
            if (!begin_streamed_download(u)) throw Error{E_ARG, "walk graph: this unit's download cannot be streamed (no window cuts, or no copy engines)"};
            stream_wait_all(u);           // every window and the bases
        } else do_download(u);
        const GraphView G = view_of(u);
        const size_t ni = G.n_ids; size_t nb[GA_N];      // nb: the bytes of each array that were downloaded
        graph_arrays(u, graph_counts(u), [&](int which, auto &h, auto &, size_t n, size_t) { nb[which] = n * sizeof(*h.p); });
        auto dup = [](const void *p, size_t bytes) { void *q = malloc(bytes + 1); if (!q) throw Error{E_ARG, "out of host memory"}; if (bytes) memcpy(q, p, bytes); return q; };
        g->n_pos = G.n_pos; g->n_ids = G.n_ids; g->n_special = G.n_special; g->n_ovf = (uint32_t)G.n_ovf; g->n_chain_str = u->n_chain_str;
        g->meta = (uint8_t *)dup(G.meta, nb[GA_META]); g->str = (char *)dup(G.str, nb[GA_STR]); g->side_xpos = (uint32_t *)dup(G.side_xpos, nb[GA_XPOS]);
        g->sp_bits = (uint64_t *)dup(G.sp_bits, nb[GA_BITS]); g->sp_rank = (uint32_t *)dup(G.sp_rank, nb[GA_RANK]);
        g->sp_node = (agx_walk_rec *)dup(G.sp_node, nb[GA_NODE]); g->sp_hop = (agx_walk_hop *)dup(G.sp_hop, nb[GA_HOP]);
        g->ovf = (uint32_t *)dup(G.ovf, nb[GA_OVF]); g->chain_str = (char *)dup(u->V.chain_str, u->n_chain_str);
        if (want_all) {                   // every id's record through the fetch path: whole rows of 64 ids a stride apart, then the rest as one row
            g->all_node = (agx_walk_rec *)malloc((ni + 1) * sizeof(agx_walknode));
            if (!g->all_node) throw Error{E_ARG, "out of host memory"};
            const agx_u32 rows = (agx_u32)(ni / 64);
            if (rows) G.fetch(G.fetch_ctx, 0, 64, rows, 64, (agx_walknode *)g->all_node);
            if (ni % 64) G.fetch(G.fetch_ctx, rows * 64u, 0, 1, (agx_u32)(ni % 64), (agx_walknode *)g->all_node + (size_t)rows * 64);
        }
        if (streamed) u->downloaded = false;      // (as agx_unit_finish leaves a streamed unit: the next finish downloads again)
    });
    if (rc != AGX_OK) agx_walk_graph_free(g);
    return rc;
}

void agx_walk_graph_free(agx_walk_graph *g) {
    if (!g) return;
    free(g->meta); free(g->str); free(g->side_xpos); free(g->sp_bits); free(g->sp_rank); free(g->sp_node); free(g->sp_hop); free(g->ovf); free(g->chain_str); free(g->all_node);
    memset(g, 0, sizeof *g);
}

// Test and inspection hook: the arrays in front of the node sweep, as the last attempt of the last build left them in HBM.  Every copy goes through the download stream
// (under its mutex, like a record fetch) into ordinary memory and is waited for there; the unit's own buffers are read, none is taken.
int agx_unit_front(agx_unit *u, agx_front *f) {
    if (!u || !f) return AGX_E_ARG;
    memset(f, 0, sizeof *f);
    const int rc = guarded(u, [&] {
        static_assert(sizeof(agx_dhit) == 40 && sizeof(agx_cmkey) == 8 && sizeof(agx_cmhead) == 16 && sizeof(agx_run) == 12, "include/agx.h describes the front's records as words");
        if (u->prm.flags & AGX_FLAG_ONE_SHOT) throw Error{E_ARG, "front: a one-shot unit gives its arrays away with its only download"};
        if (!u->built || u->trimmed || u->downloaded) throw Error{E_ARG, "front: the unit is not built (call agx_unit_build; not after agx_unit_download, agx_unit_trim or agx_unit_release)"};
        HIP_OK(hipSetDevice(u->prm.device));
        HIP_OK(wait_event(u->ev_built));
        const size_t n_pos = u->V.n_pos, nh = u->nh, nt = u->n_tiles, vbytes = codes_bytes(u) * 4;
        const agx_u32 *w = u->h_words.p;
        f->n_pos = (uint32_t)n_pos; f->n_hits = (uint32_t)nh; f->n_runs = (uint32_t)u->n_runs; f->n_cm = (uint32_t)u->n_cm; f->n_tiles = (uint32_t)nt; f->stride = u->stride;
        f->n_rows = u->stride ? (uint32_t)(vbytes / u->stride) : 0u; f->lookback = u->lookback;
        f->long_count = w[W_LONGCOUNT]; f->n_long = std::min<agx_u32>(w[W_LONGCOUNT], AGX_LONG_MAX); f->w_err = w[W_ERR]; f->w_status = w[W_STATUS];
        f->tiled = u->tiled; f->rows_diffed = u->rows_diffed; f->ref_packed = u->ref_packed; f->dense_queued = u->dense; f->swept_windows = u->front_windows;
        DeviceTurn &turn = turn_of(u->prm.device);
        std::lock_guard<std::mutex> l(turn.down_m);
        auto down = [&](auto *&dst, const void *src, size_t bytes) {
            dst = (std::remove_reference_t<decltype(dst)>)malloc(bytes + 16);
            if (!dst) throw Error{E_ARG, "out of host memory"};
            if (bytes) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, turn.down));
        };
        try {
            down(f->tile_off, u->d_tile_off.p, (nt + 1) * 4);
            HIP_OK(hipStreamSynchronize(turn.down));
            f->n_entries = f->tile_off[nt];
            if (f->n_entries > u->list_cap) throw Error{E_DEVICE, "internal: the tile lists of a converged build do not fit their buffer"};
            down(f->ref, u->d_ref.p, n_pos); down(f->vcodes, u->d_vcodes.p, (size_t)f->n_rows * u->stride); down(f->runs, u->d_runs.p, u->n_runs * sizeof(agx_run));
            down(f->cm_start, u->d_cm_start.p, (n_pos + 1) * 4); down(f->cm, u->d_cm.p, u->n_cm * sizeof(agx_cmkey)); down(f->cm_head, u->d_cm_head.p, (n_pos + 1) * sizeof(agx_cmhead));
            down(f->dhit, u->d_dhit.p, nh * sizeof(agx_dhit)); down(f->perm, u->d_perm.p, nh * 4); down(f->tile_first, u->d_tfirst.p, (nt + 1) * 4); down(f->ckey, u->d_ckey.p, nh * 4);
            down(f->tile_cnt, u->d_tile_cnt.p, (nt + 1) * 4); down(f->tile_recs, u->d_tile_recs.p, (size_t)f->n_entries * 32); down(f->long_list, u->d_long.p, (size_t)f->n_long * 4);
            HIP_OK(hipStreamSynchronize(turn.down));
        } catch (...) { (void)hipStreamSynchronize(turn.down); throw; }      // (no copy outlives the memory it lands in)
    });
    if (rc != AGX_OK) agx_front_free(f);
    return rc;
}

void agx_front_free(agx_front *f) {
    if (!f) return;
    free(f->ref); free(f->vcodes); free(f->runs); free(f->cm_start); free(f->cm); free(f->cm_head); free(f->dhit); free(f->perm); free(f->tile_first); free(f->ckey);
    free(f->tile_cnt); free(f->tile_off); free(f->tile_recs); free(f->long_list);
    memset(f, 0, sizeof *f);
}

int agx_run_unit(const agx_params *p, const char *tmp_dir, int unit, int write_files, agx_result *r, char *err, size_t err_len) {
    return agx_run_unit_shared(p, tmp_dir, unit, write_files, nullptr, r, err, err_len);
}

int agx_run_unit_shared(const agx_params *p, const char *tmp_dir, int unit, int write_files, const agx_reads *reads, agx_result *r, char *err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    agx_unit *u = nullptr;
    agx_params once; if (p) { once = *p; once.flags |= AGX_FLAG_ONE_SHOT; }      // created, loaded, uploaded once, finished and destroyed here: the download may land in the dead staged inputs
    int rc = agx_unit_create(p ? &once : nullptr, &u);
    if (rc != AGX_OK) { if (err && err_len) snprintf(err, err_len, "%s", rc == AGX_E_NOGPU ? "no HIP device" : "bad parameters"); return rc; }
    rc = agx_unit_load_files_shared(u, tmp_dir, unit, reads);
    if (rc == AGX_OK) rc = agx_unit_upload(u);
    if (rc == AGX_OK) rc = agx_unit_build(u);
    if (rc == AGX_OK) rc = agx_unit_finish(u, r);
    if (rc == AGX_OK && write_files)
        rc = guarded(u, [&] {
            const std::string d = tmp_dir, s = std::to_string(unit);
            write_file(d + "/_initial_contigs." + s + ".fa", std::string(r->initial_contigs, r->initial_len));
            write_file(d + "/_pre_extended_contigs." + s + ".fa", std::string(r->pre_extended, r->pre_len));
            write_file(d + "/_extended_contigs." + s + ".fa", std::string(r->extended, r->extended_len));
        });
    if (rc != AGX_OK && err && err_len) snprintf(err, err_len, "%s", agx_unit_error(u));
    if (rc != AGX_OK && r) agx_result_free(r);          // (a failed write of the three files leaves nothing allocated behind)
    agx_unit_destroy(u);
    return rc;
}

}  // extern "C"
