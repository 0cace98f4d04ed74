"""aligngraph_amd — ctypes binding of libagx.so (include/agx.h), the MI355X engine for AlignGraph's per-unit
graph build + extend path (reference seam: AlignGraph/AlignGraph.cpp:4765-4783).

The library is the product; this module only loads it, mirrors the C structs and raises on error codes.
There is no CPU fallback: without a HIP device `Unit(...)` raises AgxError(AGX_E_NOGPU).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AGX_LIB_PATH", os.path.join(_HERE, "libagx.so"))   # override only for kernel A/B experiments

AGX_OK, AGX_E_IO, AGX_E_FORMAT, AGX_E_UNSUPPORTED, AGX_E_ALIGNMENT, AGX_E_DEVICE, AGX_E_ARG, AGX_E_OVERFLOW, AGX_E_NOGPU = 0, -1, -2, -3, -4, -5, -6, -7, -8
AGX_FLAG_KEEP_COUNTS = 1
AGX_FLAG_SPARSE_MIN = 2
AGX_FLAG_TIME_SECTIONS = 4
AGX_FLAG_ONE_SHOT = 8
AGX_FLAG_KEEP_PATHS = 16
AGX_FLAG_EDGE_SUPPORT = 32

# every symbol include/agx.h declares (tests check that the built library exports all of them)
EXPORTS = [
    "agx_version", "agx_device_count", "agx_device_memory", "agx_selftest_scan", "agx_unit_create", "agx_unit_destroy", "agx_unit_error", "agx_unit_set_reference",
    "agx_unit_set_contig_threads", "agx_unit_push_pairs", "agx_unit_load_files", "agx_unit_upload", "agx_unit_build", "agx_unit_download",
    "agx_unit_finish", "agx_result_free", "agx_unit_stats", "agx_unit_graph", "agx_graph_free", "agx_run_unit",
    "agx_reads_open", "agx_reads_close", "agx_unit_load_files_shared", "agx_run_unit_shared",
    "agx_unit_stage", "agx_unit_release", "agx_pool_trim", "agx_unit_cache_build", "agx_unit_cache_save", "agx_unit_hbm_needed",
    "agx_unit_trim", "agx_unit_unitigs", "agx_unit_unitigs_region", "agx_unitigs_free", "agx_unitigs_gfa", "agx_text_free",
    "agx_unit_walk_graph", "agx_walk_graph_free", "agx_unit_front", "agx_front_free",
    "agx_unit_unitigs_mapped", "agx_idmap_free", "agx_unit_walk_paths", "agx_walk_paths_free", "agx_unitigs_paths_gfa", "agx_unit_reprune",
    "agx_unit_edge_support", "agx_edge_support_free", "agx_unit_unitigs_support", "agx_link_support_free", "agx_unitigs_gfa_support",
    "agx_unit_walk_evidence", "agx_walk_evidence_free", "agx_walk_evidence_bed",
    "agx_unit_edge_reads", "agx_edge_reads_free", "agx_edge_reads_tsv",
    "agx_unit_pair_span", "agx_pair_span_free", "agx_unit_walk_span", "agx_walk_span_free", "agx_walk_span_bed",
    "agx_unit_mate_links", "agx_mate_links_free", "agx_mate_links_tsv",
    "agx_unit_bubbles", "agx_unitigs_bubbles", "agx_bubbles_free", "agx_bubbles_tsv",
    "agx_test_scan", "agx_test_zero", "agx_test_copy_out", "agx_test_poison",
]


class Params(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint32), ("insert_variation", ctypes.c_uint32), ("coverage", ctypes.c_uint32),
                ("batch", ctypes.c_uint32), ("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class Run(ctypes.Structure):
    _fields_ = [("q", ctypes.c_uint32), ("t", ctypes.c_uint32), ("n", ctypes.c_uint32)]


class Hit(ctypes.Structure):
    _fields_ = [("slot1", ctypes.c_uint32), ("pos1", ctypes.c_uint32), ("pos2", ctypes.c_uint32), ("runs1", ctypes.c_uint32),
                ("runs2", ctypes.c_uint32), ("nruns1", ctypes.c_uint16), ("nruns2", ctypes.c_uint16), ("len", ctypes.c_uint16),
                ("rev1", ctypes.c_uint8), ("rev2", ctypes.c_uint8), ("back", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]


class ContiMer(ctypes.Structure):
    _fields_ = [("cid", ctypes.c_uint32), ("coff", ctypes.c_uint32), ("next_off", ctypes.c_uint32), ("next_item", ctypes.c_uint32),
                ("nuc", ctypes.c_char), ("pad", ctypes.c_char * 3)]


class PairBatch(ctypes.Structure):
    _fields_ = [("hits", ctypes.POINTER(Hit)), ("n_hits", ctypes.c_uint64), ("runs", ctypes.POINTER(Run)), ("n_runs", ctypes.c_uint64),
                ("bases", ctypes.c_char_p), ("stride", ctypes.c_uint32), ("n_slots", ctypes.c_uint32)]


class Result(ctypes.Structure):
    _fields_ = [("initial_contigs", ctypes.c_void_p), ("initial_len", ctypes.c_size_t), ("pre_extended", ctypes.c_void_p),
                ("pre_len", ctypes.c_size_t), ("extended", ctypes.c_void_p), ("extended_len", ctypes.c_size_t)]


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_pos", "n_ref", "n_hits", "n_runs", "n_nodes", "n_tiles", "n_tile_entries", "n_big_tiles",
                                                "n_edge_overflow", "pairs_in_file", "sam_line_pairs")] + \
               [(n, ctypes.c_double) for n in ("ms_parse", "ms_thread", "ms_upload", "ms_prep", "ms_bin", "ms_node_sweep", "ms_node_big",
                                                "ms_edge_sweep", "ms_compact", "ms_download", "ms_walk")] + \
               [("node_sweep_launches", ctypes.c_uint32), ("edge_sweep_launches", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("n_walk_ids", "n_special", "n_fetched", "download_bytes")] + \
               [(n, ctypes.c_double) for n in ("ms_edge_fast", "ms_edge_slow")] + [("n_mid_tiles", ctypes.c_uint64), ("ms_build_span", ctypes.c_double)] + \
               [(n, ctypes.c_double) for n in ("ms_stage", "ms_upload_dev")] + \
               [(n, ctypes.c_uint64) for n in ("upload_bytes", "device_bytes", "pinned_bytes_cached", "device_bytes_cached", "n_spilled")] + \
               [("build_attempts", ctypes.c_uint32), ("from_cache", ctypes.c_uint32), ("dense_lists", ctypes.c_uint32), ("rows_by_reference", ctypes.c_uint32)] + \
               [("n_edge_slow", ctypes.c_uint64), ("reprune_attempts", ctypes.c_uint32), ("ms_reprune", ctypes.c_double)] + \
               [("ms_edge_support", ctypes.c_double), ("n_support_events", ctypes.c_uint64), ("ms_walk_evidence", ctypes.c_double), ("ms_edge_reads", ctypes.c_double)] + \
               [("ms_pair_span", ctypes.c_double), ("ms_walk_span", ctypes.c_double)]


class Graph(ctypes.Structure):
    _fields_ = [("n_pos", ctypes.c_uint32), ("n_nodes", ctypes.c_uint32), ("n_edges", ctypes.c_uint32),
                ("node_start", ctypes.POINTER(ctypes.c_uint32)), ("node_key", ctypes.POINTER(ctypes.c_uint32)),
                ("node_cnt", ctypes.POINTER(ctypes.c_int32)), ("node_slen", ctypes.POINTER(ctypes.c_uint32)),
                ("edge_start", ctypes.POINTER(ctypes.c_uint32)), ("edge_dst", ctypes.POINTER(ctypes.c_uint32))]


class Unitigs(ctypes.Structure):
    _fields_ = [("n_segs", ctypes.c_uint32), ("n_links", ctypes.c_uint32), ("n_bases", ctypes.c_uint64),
                ("head_pos", ctypes.POINTER(ctypes.c_uint32)), ("head_var", ctypes.POINTER(ctypes.c_uint32)), ("n_nodes", ctypes.POINTER(ctypes.c_uint32)),
                ("last_pos", ctypes.POINTER(ctypes.c_uint32)), ("coverage", ctypes.POINTER(ctypes.c_uint64)), ("seq_off", ctypes.POINTER(ctypes.c_uint64)),
                ("seq", ctypes.c_void_p), ("link_from", ctypes.POINTER(ctypes.c_uint32)), ("link_to", ctypes.POINTER(ctypes.c_uint32))]


EDGE_READS_EDGE = ("src_pos", "src_var", "dst_pos", "dst_var", "support")


class EdgeSupport(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint32), ("n_edges", ctypes.c_uint32), ("n_events", ctypes.c_uint64), ("n_contributions", ctypes.c_uint64)] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("edge_start", "edge_dst", "edge_cnt")]


class EdgeReads(ctypes.Structure):
    _fields_ = [("n_edges", ctypes.c_uint32), ("n_hits", ctypes.c_uint64)] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in EDGE_READS_EDGE] + [("hit_off", ctypes.POINTER(ctypes.c_uint64)), ("hit", ctypes.POINTER(ctypes.c_uint32))]


class IdMap(ctypes.Structure):
    _fields_ = [("n_runs", ctypes.c_uint32), ("n_pos", ctypes.c_uint32), ("n_ids", ctypes.c_uint32)] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("id_first", "id_last", "seg", "rank_first")]


class WalkPaths(ctypes.Structure):
    _fields_ = [("n_recs", ctypes.c_uint32), ("n_stretches", ctypes.c_uint64), ("rec_len", ctypes.POINTER(ctypes.c_uint64)), ("st_off", ctypes.POINTER(ctypes.c_uint64)),
                ("id_first", ctypes.POINTER(ctypes.c_uint32)), ("id_last", ctypes.POINTER(ctypes.c_uint32)), ("base_off", ctypes.POINTER(ctypes.c_uint64)),
                ("joined", ctypes.POINTER(ctypes.c_uint8))]


class WalkEvidence(ctypes.Structure):
    _fields_ = [("n_recs", ctypes.c_uint32), ("n_intervals", ctypes.c_uint32), ("n_graph_bases", ctypes.c_uint64), ("n_steps", ctypes.c_uint64), ("n_steps_without_edge", ctypes.c_uint64)] + \
               [(n, ctypes.POINTER(ctypes.c_uint64)) for n in ("rec_graph_bases", "rec_steps", "rec_depth_sum")] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("rec_depth_min", "rec_depth_min_at", "rec_step_min", "rec_step_min_at",
                                                               "iv_rec", "iv_first", "iv_last", "iv_depth_min", "iv_step_min")] + \
               [("rec_lo", ctypes.c_uint32), ("rec_hi", ctypes.c_uint32), ("n_track", ctypes.c_uint64), ("track_off", ctypes.POINTER(ctypes.c_uint64))] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("depth", "votes", "step")]


class PairSpan(ctypes.Structure):
    _fields_ = [("pos_lo", ctypes.c_uint32), ("pos_hi", ctypes.c_uint32), ("n_kept", ctypes.c_uint64), ("n_fragments", ctypes.c_uint64), ("n_outside", ctypes.c_uint64),
                ("span", ctypes.POINTER(ctypes.c_uint32)), ("cross", ctypes.POINTER(ctypes.c_uint32))]


class WalkSpan(ctypes.Structure):
    _fields_ = [("n_recs", ctypes.c_uint32), ("n_intervals", ctypes.c_uint32)] + [(n, ctypes.c_uint64) for n in ("n_graph_bases", "n_steps", "n_jump_steps", "n_steps_not_forward")] + \
               [(n, ctypes.POINTER(ctypes.c_uint64)) for n in ("rec_graph_bases", "rec_steps", "rec_span_sum")] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("rec_span_min", "rec_span_min_at", "rec_step_min", "rec_step_min_at",
                                                               "iv_rec", "iv_first", "iv_last", "iv_span_min", "iv_step_min")] + \
               [("rec_lo", ctypes.c_uint32), ("rec_hi", ctypes.c_uint32), ("n_track", ctypes.c_uint64), ("track_off", ctypes.POINTER(ctypes.c_uint64))] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("pos", "span", "step")]


class MateLinks(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("n_kept", "n_outside", "n_fragments", "n_unowned", "n_inside", "n_open", "n_link_pairs", "n_links_all", "n_owned", "n_shadowed")] + \
               [(n, ctypes.c_uint32) for n in ("n_recs", "n_links", "n_passes", "n_slots")] + [("ms", ctypes.c_double)] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("rec_inside", "rec_open_left", "rec_open_right", "rec_links_out", "rec_links_in", "a", "b", "n_pairs")] + \
               [("len_sum", ctypes.POINTER(ctypes.c_uint64))] + [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("lo_min", "lo_max", "hi_min", "hi_max")]


class Bubbles(ctypes.Structure):
    _fields_ = [("n_segs", ctypes.c_uint32), ("n_links", ctypes.c_uint32)] + \
               [(n, ctypes.c_uint64) for n in ("n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared")] + \
               [(n, ctypes.c_uint32) for n in ("longest_branch", "max_nodes", "has_support", "n_bubbles", "n_branches")] + \
               [("n_bases", ctypes.c_uint64), ("bytes_down", ctypes.c_uint64), ("ms", ctypes.c_double)] + \
               [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("src_pos", "src_var", "src_last", "sink_pos", "sink_var", "br_off", "br_pos", "br_var", "br_nodes")] + \
               [(n, ctypes.POINTER(ctypes.c_uint64)) for n in ("br_cov", "br_seq_off")] + [(n, ctypes.POINTER(ctypes.c_uint32)) for n in ("br_sup_in", "br_sup_out")] + \
               [("seq", ctypes.c_void_p)]


TOTALS_BUBBLES = ("n_segs", "n_links", "n_forks", "n_bubbles_all", "n_tip", "n_nested", "n_sinks_differ", "n_sink_shared", "longest_branch", "max_nodes")
BUBBLE_BUBBLES = ("src_pos", "src_var", "src_last", "sink_pos", "sink_var")
BRANCH_BUBBLES = ("br_pos", "br_var", "br_nodes", "br_cov")
TOTALS_LINKS = ("n_kept", "n_outside", "n_fragments", "n_unowned", "n_inside", "n_open", "n_link_pairs", "n_links_all", "n_owned", "n_shadowed", "n_passes", "n_slots")
REC_LINKS = ("rec_inside", "rec_open_left", "rec_open_right", "rec_links_out", "rec_links_in")
LINK_LINKS = ("a", "b", "n_pairs", "len_sum", "lo_min", "lo_max", "hi_min", "hi_max")
REC_SPAN = ("rec_graph_bases", "rec_steps", "rec_span_sum", "rec_span_min", "rec_span_min_at", "rec_step_min", "rec_step_min_at")
IV_SPAN = ("iv_rec", "iv_first", "iv_last", "iv_span_min", "iv_step_min")
REC_EVIDENCE = ("rec_graph_bases", "rec_steps", "rec_depth_sum", "rec_depth_min", "rec_depth_min_at", "rec_step_min", "rec_step_min_at")
IV_EVIDENCE = ("iv_rec", "iv_first", "iv_last", "iv_depth_min", "iv_step_min")


class WalkGraph(ctypes.Structure):
    _fields_ = [("want_all_node", ctypes.c_uint32), ("n_pos", ctypes.c_uint32), ("n_ids", ctypes.c_uint32), ("n_special", ctypes.c_uint32), ("n_ovf", ctypes.c_uint32),
                ("n_chain_str", ctypes.c_uint64), ("meta", ctypes.c_void_p), ("str", ctypes.c_void_p), ("side_xpos", ctypes.c_void_p), ("sp_bits", ctypes.c_void_p),
                ("sp_rank", ctypes.c_void_p), ("sp_node", ctypes.c_void_p), ("sp_hop", ctypes.c_void_p), ("ovf", ctypes.c_void_p), ("chain_str", ctypes.c_void_p),
                ("all_node", ctypes.c_void_p)]


# numpy layouts of agx_walk_rec and agx_walk_hop
WALK_RECORD = [("next", "<u4", (4,)), ("off0", "<u4"), ("xpos", "<u4"), ("sref_slot", "<u4"), ("sref_qlen", "<u4")]
WALK_HOP = [("str_off", "<u4"), ("len", "<u4"), ("end_pos", "<u4")]


def _arr(p, n, dt):
    """n entries at p as a numpy array of its own: p is a typed ctypes pointer, whose entries are converted to dt, or an address (a c_void_p field) of entries of dt."""
    import numpy as np
    if not p or not n:
        return np.zeros(0, dt)
    if isinstance(p, int):
        return np.frombuffer(ctypes.string_at(p, n * np.dtype(dt).itemsize), dtype=dt).copy()
    return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)


def _text(fn, *args, what):
    """The text one of the library's writers makes of args, as bytes; what: the message when it refuses them."""
    p, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    rc = fn(*args, ctypes.byref(p), ctypes.byref(n))
    if rc != AGX_OK:
        raise AgxError(rc, what)
    try:
        return ctypes.string_at(p, n.value) if n.value else b""
    finally:
        lib().agx_text_free(p)


def walk_graph_arrays(g):
    """An agx_walk_graph-shaped ctypes struct (this library's, or the test executor's) as a dict of numpy arrays; str and chain_str as bytes."""
    ni, nw = g.n_ids, g.n_ids // 64 + 1
    return {"n_pos": g.n_pos, "n_ids": ni, "n_special": g.n_special, "meta": _arr(g.meta, ni, "u1"), "str": ctypes.string_at(g.str, ni) if g.str else b"",
            "side_xpos": _arr(g.side_xpos, ni - g.n_pos, "<u4"), "sp_bits": _arr(g.sp_bits, nw, "<u8"), "sp_rank": _arr(g.sp_rank, nw, "<u4"),
            "sp_node": _arr(g.sp_node, g.n_special, WALK_RECORD), "sp_hop": _arr(g.sp_hop, g.n_special, WALK_HOP), "ovf": _arr(g.ovf, g.n_ovf * 2, "<u4").reshape(-1, 2),
            "chain_str": ctypes.string_at(g.chain_str, g.n_chain_str) if g.chain_str else b"",
            "all_node": _arr(g.all_node, ni, WALK_RECORD) if g.all_node else None}


class Front(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("n_pos", "n_hits", "n_runs", "n_cm", "n_tiles", "stride", "n_rows", "lookback", "n_entries", "long_count", "n_long",
                                                "w_err", "w_status", "tiled", "rows_diffed", "ref_packed", "dense_queued", "swept_windows")] + \
               [(n, ctypes.c_void_p) for n in ("ref", "vcodes", "runs", "cm_start", "cm", "cm_head", "dhit", "perm", "tile_first", "ckey", "tile_cnt", "tile_off",
                                                "tile_recs", "long_list")]


# numpy layouts of the front's records (agx_front, include/agx.h)
FRONT_DHIT = [("a_t0", "<u4"), ("b_t0", "<u4"), ("a_runs", "<u4"), ("b_runs", "<u4"), ("a_slot", "<u4"), ("len", "<u2"), ("jstar", "<u2"), ("a_nruns", "<u2"), ("b_nruns", "<u2"),
              ("flags", "<u4"), ("x_lo", "<u4"), ("x_hi", "<u4")]
FRONT_LREC = [("qoff1", "<u4"), ("boff1", "<u4"), ("qoff2", "<u4"), ("boff2", "<u4"), ("slot", "<u4"), ("lenjs", "<u4"), ("geo", "<u4"), ("hit", "<u4")]
FRONT_RUN = [("q", "<u4"), ("t", "<u4"), ("n", "<u4")]
FRONT_CMKEY = [("cid", "<u4"), ("coff", "<u4")]
FRONT_CMHEAD = [("cid", "<u4"), ("coff", "<u4"), ("n", "<u4"), ("start", "<u4")]


def front_arrays(f):
    """An agx_front-shaped ctypes struct (this library's, or the test executor's) as a dict: the counts and form flags as ints, ref as bytes, the arrays as numpy arrays
    (records as structured arrays with the fields of FRONT_*; vcodes as [n_rows, stride])."""
    out = {n: int(getattr(f, n)) for n, t in Front._fields_ if t is ctypes.c_uint32}
    nt = f.n_tiles
    out.update({"ref": ctypes.string_at(f.ref, f.n_pos) if f.ref else b"", "vcodes": _arr(f.vcodes, f.n_rows * f.stride, "u1").reshape(f.n_rows, f.stride),
                "runs": _arr(f.runs, f.n_runs, FRONT_RUN), "cm_start": _arr(f.cm_start, f.n_pos + 1, "<u4"), "cm": _arr(f.cm, f.n_cm, FRONT_CMKEY),
                "cm_head": _arr(f.cm_head, f.n_pos + 1, FRONT_CMHEAD), "dhit": _arr(f.dhit, f.n_hits, FRONT_DHIT), "perm": _arr(f.perm, f.n_hits, "<u4"),
                "tile_first": _arr(f.tile_first, nt + 1, "<u4"), "ckey": _arr(f.ckey, f.n_hits, "<u4"), "tile_cnt": _arr(f.tile_cnt, nt + 1, "<u4"),
                "tile_off": _arr(f.tile_off, nt + 1, "<u4"), "tile_recs": _arr(f.tile_recs, f.n_entries, FRONT_LREC), "long_list": _arr(f.long_list, f.n_long, "<u4")})
    return out


class AgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("agx error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


_lib = None


def lib():
    """Loads libagx.so (build it first with `python -m aligngraph_amd.build` or __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError("%s is missing: run `python aligngraph_amd/build.py` (needs hipcc)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.agx_version.restype = ctypes.c_char_p
        L.agx_device_count.restype = ctypes.c_int
        L.agx_unit_create.argtypes = [ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_void_p)]
        L.agx_unit_destroy.argtypes = [ctypes.c_void_p]
        L.agx_unit_destroy.restype = None
        L.agx_unit_error.argtypes = [ctypes.c_void_p]
        L.agx_unit_error.restype = ctypes.c_char_p
        L.agx_unit_set_reference.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32]
        L.agx_unit_set_contig_threads.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                                  ctypes.POINTER(ContiMer), ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
        L.agx_unit_push_pairs.argtypes = [ctypes.c_void_p, ctypes.POINTER(PairBatch)]
        L.agx_device_memory.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.agx_selftest_scan.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        L.agx_test_scan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.agx_test_zero.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        L.agx_test_copy_out.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)]
        L.agx_test_poison.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        L.agx_unit_load_files.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        L.agx_reads_open.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_size_t]
        L.agx_reads_close.argtypes = [ctypes.c_void_p]
        L.agx_reads_close.restype = None
        L.agx_unit_load_files_shared.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
        L.agx_unit_cache_build.argtypes = [ctypes.POINTER(Params), ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        L.agx_unit_cache_save.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        L.agx_unit_hbm_needed.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.agx_unit_trim.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.agx_pool_trim.argtypes = [ctypes.c_int]
        L.agx_pool_trim.restype = None
        for f in ("agx_unit_upload", "agx_unit_build", "agx_unit_download", "agx_unit_stage", "agx_unit_release"):
            getattr(L, f).argtypes = [ctypes.c_void_p]
        L.agx_unit_reprune.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.agx_unit_finish.argtypes = [ctypes.c_void_p, ctypes.POINTER(Result)]
        L.agx_result_free.argtypes = [ctypes.POINTER(Result)]
        L.agx_result_free.restype = None
        L.agx_unit_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats)]
        L.agx_unit_graph.argtypes = [ctypes.c_void_p, ctypes.POINTER(Graph)]
        L.agx_graph_free.argtypes = [ctypes.POINTER(Graph)]
        L.agx_graph_free.restype = None
        L.agx_unit_walk_graph.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(WalkGraph)]
        L.agx_walk_graph_free.argtypes = [ctypes.POINTER(WalkGraph)]
        L.agx_walk_graph_free.restype = None
        L.agx_unit_front.argtypes = [ctypes.c_void_p, ctypes.POINTER(Front)]
        L.agx_front_free.argtypes = [ctypes.POINTER(Front)]
        L.agx_front_free.restype = None
        L.agx_unit_unitigs.argtypes = [ctypes.c_void_p, ctypes.POINTER(Unitigs)]
        L.agx_unit_unitigs_region.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Unitigs)]
        L.agx_unit_unitigs_mapped.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Unitigs), ctypes.POINTER(IdMap)]
        L.agx_idmap_free.argtypes = [ctypes.POINTER(IdMap)]
        L.agx_idmap_free.restype = None
        L.agx_unit_walk_paths.argtypes = [ctypes.c_void_p, ctypes.POINTER(WalkPaths)]
        L.agx_walk_paths_free.argtypes = [ctypes.POINTER(WalkPaths)]
        L.agx_walk_paths_free.restype = None
        L.agx_unitigs_paths_gfa.argtypes = [ctypes.POINTER(Unitigs), ctypes.POINTER(IdMap), ctypes.POINTER(WalkPaths), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_unitigs_free.argtypes = [ctypes.POINTER(Unitigs)]
        L.agx_unitigs_free.restype = None
        L.agx_unitigs_gfa.argtypes = [ctypes.POINTER(Unitigs), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_unit_edge_support.argtypes = [ctypes.c_void_p, ctypes.POINTER(EdgeSupport)]
        L.agx_edge_support_free.argtypes = [ctypes.POINTER(EdgeSupport)]
        L.agx_edge_support_free.restype = None
        L.agx_unit_unitigs_support.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Unitigs),
                                               ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)), ctypes.POINTER(IdMap)]
        L.agx_link_support_free.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
        L.agx_link_support_free.restype = None
        L.agx_unitigs_gfa_support.argtypes = [ctypes.POINTER(Unitigs), ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_text_free.argtypes = [ctypes.c_void_p]
        L.agx_unit_walk_evidence.argtypes = [ctypes.c_void_p, ctypes.POINTER(WalkPaths)] + [ctypes.c_uint32] * 5 + [ctypes.POINTER(WalkEvidence)]
        L.agx_walk_evidence_free.argtypes = [ctypes.POINTER(WalkEvidence)]
        L.agx_walk_evidence_free.restype = None
        L.agx_walk_evidence_bed.argtypes = [ctypes.POINTER(WalkEvidence), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_unit_pair_span.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(PairSpan)]
        L.agx_pair_span_free.argtypes = [ctypes.POINTER(PairSpan)]
        L.agx_pair_span_free.restype = None
        L.agx_unit_walk_span.argtypes = [ctypes.c_void_p, ctypes.POINTER(WalkPaths)] + [ctypes.c_uint32] * 4 + [ctypes.POINTER(WalkSpan)]
        L.agx_walk_span_free.argtypes = [ctypes.POINTER(WalkSpan)]
        L.agx_walk_span_free.restype = None
        L.agx_walk_span_bed.argtypes = [ctypes.POINTER(WalkSpan), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_unit_mate_links.argtypes = [ctypes.c_void_p, ctypes.POINTER(WalkPaths), ctypes.c_uint32, ctypes.POINTER(MateLinks)]
        L.agx_mate_links_free.argtypes = [ctypes.POINTER(MateLinks)]
        L.agx_mate_links_free.restype = None
        L.agx_mate_links_tsv.argtypes = [ctypes.POINTER(MateLinks), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_text_free.restype = None
        L.agx_unit_edge_reads.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(EdgeReads)]
        L.agx_edge_reads_free.argtypes = [ctypes.POINTER(EdgeReads)]
        L.agx_edge_reads_free.restype = None
        L.agx_unit_bubbles.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] * 5 + [ctypes.POINTER(Bubbles)]
        L.agx_unitigs_bubbles.argtypes = [ctypes.POINTER(Unitigs), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(Bubbles)]
        L.agx_bubbles_free.argtypes = [ctypes.POINTER(Bubbles)]
        L.agx_bubbles_free.restype = None
        L.agx_bubbles_tsv.argtypes = [ctypes.POINTER(Bubbles), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_edge_reads_tsv.argtypes = [ctypes.POINTER(EdgeReads), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.agx_run_unit.argtypes = [ctypes.POINTER(Params), ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Result), ctypes.c_char_p, ctypes.c_size_t]
        _lib = L
    return _lib


def device_memory(device=0):
    """(free, total) bytes of HBM on one device (hipMemGetInfo)."""
    f, t = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib().agx_device_memory(device, ctypes.byref(f), ctypes.byref(t))
    if rc != AGX_OK:
        raise AgxError(rc, "agx_device_memory failed")
    return f.value, t.value


def device_count():
    return lib().agx_device_count()


def pool_trim(device=0, host=True, retire_host=False):
    """Frees what the library's memory caches hold: HBM blocks of `device` (>= 0) and (host=True) the pinned host blocks.  retire_host: the
    cached pinned blocks are only taken out of circulation (later allocations map and register fresh memory); a pool_trim(host=True) unmaps them."""
    if device >= 0:
        lib().agx_pool_trim(device)
    if retire_host:
        lib().agx_pool_trim(-2)
    elif host:
        lib().agx_pool_trim(-1)


def _take(res):
    out = {"initial": ctypes.string_at(res.initial_contigs, res.initial_len) if res.initial_contigs else b"",
           "pre": ctypes.string_at(res.pre_extended, res.pre_len) if res.pre_extended else b"",
           "extended": ctypes.string_at(res.extended, res.extended_len) if res.extended else b""}
    lib().agx_result_free(ctypes.byref(res))
    return out


class ResultViews:
    """The three output buffers of agx_unit_finish without a Python copy: view(name) is a numpy uint8 array over the C buffer (valid until
    free()), bytes(name) a copy.  A loop that runs many units from several threads should not hold the interpreter lock for megabytes of
    byte-string copies per unit (bench.py)."""
    _FIELDS = {"initial": ("initial_contigs", "initial_len"), "pre": ("pre_extended", "pre_len"), "extended": ("extended", "extended_len")}

    def __init__(self, res):
        self._res = res

    def view(self, name):
        import numpy as np
        p, n = (getattr(self._res, f) for f in self._FIELDS[name])
        if not p or not n:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))

    def bytes(self, name):
        p, n = (getattr(self._res, f) for f in self._FIELDS[name])
        return ctypes.string_at(p, n) if p else b""

    def free(self):
        if self._res is not None:
            lib().agx_result_free(ctypes.byref(self._res))
            self._res = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Reads:
    """tmp/_reads.fa mapped and indexed once (agx_reads); pass it to Unit.load_files of every unit of the run."""

    def __init__(self, path):
        self._h = ctypes.c_void_p()
        err = ctypes.create_string_buffer(512)
        rc = lib().agx_reads_open(path.encode(), ctypes.byref(self._h), err, 512)
        if rc != AGX_OK:
            self._h = ctypes.c_void_p()
            raise AgxError(rc, err.value.decode(errors="replace"))

    def close(self):
        if self._h:
            lib().agx_reads_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Unit:
    """One reference unit (chromosome or --part slice): the body of the reference's unit loop, AG:4765-4783."""

    def __init__(self, k=5, insert_variation=50, coverage=20, batch=0, device=0, keep_counts=False, flags=0, keep_paths=False, edge_support=False):
        self._h = ctypes.c_void_p()
        self.params = Params(k, insert_variation, coverage, batch, device, (AGX_FLAG_KEEP_COUNTS if keep_counts else 0) | (AGX_FLAG_KEEP_PATHS if keep_paths else 0) |
                             (AGX_FLAG_EDGE_SUPPORT if edge_support else 0) | flags)
        rc = lib().agx_unit_create(ctypes.byref(self.params), ctypes.byref(self._h))
        if rc != AGX_OK:
            self._h = ctypes.c_void_p()
            raise AgxError(rc, "no HIP device (libagx has no CPU path)" if rc == AGX_E_NOGPU else "agx_unit_create failed")

    def _check(self, rc):
        if rc != AGX_OK:
            raise AgxError(rc, lib().agx_unit_error(self._h).decode(errors="replace"))

    def close(self):
        if self._h:
            lib().agx_unit_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_files(self, tmp_dir, unit, reads=None):
        """reads: an optional Reads (tmp/_reads.fa opened once for all units of a run)."""
        self._check(lib().agx_unit_load_files_shared(self._h, tmp_dir.encode(), unit, reads._h if reads is not None else None))

    def cache_save(self, tmp_dir, unit):
        """Writes tmp_dir/_agx_unit.<unit>.bin from this unit (just loaded from the text files of tmp_dir, unit)."""
        self._check(lib().agx_unit_cache_save(self._h, tmp_dir.encode(), unit))

    def stage(self):
        self._check(lib().agx_unit_stage(self._h))

    def hbm_needed(self):
        """HBM the upload of this (loaded) unit will take at its first-guess capacities: what AlignGraph_amd admits units to a device by."""
        v = ctypes.c_uint64(0)
        self._check(lib().agx_unit_hbm_needed(self._h, ctypes.byref(v)))
        return v.value

    def upload(self):
        self._check(lib().agx_unit_upload(self._h))

    def trim(self):
        """After download(): the part of the unit's HBM that the host walk cannot ask for goes back to the device's memory region (agx_unit_trim); returns the bytes given back."""
        v = ctypes.c_uint64(0)
        self._check(lib().agx_unit_trim(self._h, ctypes.byref(v)))
        return v.value

    def release(self):
        """HBM and download buffers back to the library's caches; the staged inputs stay (upload again = a new unit)."""
        self._check(lib().agx_unit_release(self._h))

    def build(self):
        self._check(lib().agx_unit_build(self._h))

    def reprune(self, coverage):
        """Re-prunes the built unit at another coverage without building it again (agx_unit_reprune; needs keep_counts): afterwards the unit is what build() leaves on a
        unit created with that coverage, and params.coverage follows, so gfa(region=...) without a threshold keeps meaning "the unit's own coverage"."""
        if not 0 <= int(coverage) <= 0xFFFFFFFF:
            raise AgxError(AGX_E_ARG, "reprune: coverage is an unsigned 32-bit number")
        self._check(lib().agx_unit_reprune(self._h, int(coverage)))
        self.params.coverage = int(coverage)

    def download(self):
        self._check(lib().agx_unit_download(self._h))

    def finish(self):
        r = Result()
        self._check(lib().agx_unit_finish(self._h, ctypes.byref(r)))
        return _take(r)

    def finish_views(self):
        r = Result()
        self._check(lib().agx_unit_finish(self._h, ctypes.byref(r)))
        return ResultViews(r)

    def stats(self):
        s = Stats()
        self._check(lib().agx_unit_stats(self._h, ctypes.byref(s)))
        return {n: getattr(s, n) for n, _ in Stats._fields_}

    def graph(self):
        g = Graph()
        self._check(lib().agx_unit_graph(self._h, ctypes.byref(g)))

        out = {"n_pos": g.n_pos, "n_nodes": g.n_nodes, "n_edges": g.n_edges,
               "node_start": _arr(g.node_start, g.n_pos + 1, "uint32"), "node_key": _arr(g.node_key, g.n_nodes * 6, "uint32").reshape(-1, 6),
               "node_cnt": _arr(g.node_cnt, g.n_nodes * 6, "int32").reshape(-1, 6), "node_slen": _arr(g.node_slen, g.n_nodes, "uint32"),
               "edge_start": _arr(g.edge_start, g.n_nodes + 1, "uint32"), "edge_dst": _arr(g.edge_dst, g.n_edges, "uint32")}
        lib().agx_graph_free(ctypes.byref(g))
        return out

    def walk_graph(self, streamed=False, all_node=False):
        """Test and inspection hook (agx_unit_walk_graph): the walk graph as the walk would be handed it, after a whole download in the one-piece form
        (streamed=False) or the windowed one (streamed=True); all_node: every id's record through the fetch path as well.  The unit stays usable."""
        g = WalkGraph()
        g.want_all_node = 1 if all_node else 0
        self._check(lib().agx_unit_walk_graph(self._h, 1 if streamed else 0, ctypes.byref(g)))
        try:
            return walk_graph_arrays(g)
        finally:
            lib().agx_walk_graph_free(ctypes.byref(g))

    def front(self):
        """Test and inspection hook (agx_unit_front): what the device holds in front of the node sweep after build() — the expanded inputs, the derived hit records in the
        device's order, the tile histogram, offsets and lists — as front_arrays() lays it out.  Before download(), trim() and release(); the unit stays usable."""
        f = Front()
        self._check(lib().agx_unit_front(self._h, ctypes.byref(f)))
        try:
            return front_arrays(f)
        finally:
            lib().agx_front_free(ctypes.byref(f))

    def _window(self, region, min_coverage):
        """(lo, hi, coverage) of a region export: every position without a region, the unit's own coverage without a threshold."""
        lo, hi = region if region is not None else (0, self.stats()["n_pos"])
        cov = self.params.coverage if min_coverage is None else min_coverage
        for v in (lo, hi, cov):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise AgxError(AGX_E_ARG, "unitigs: region bounds and min_coverage are unsigned 32-bit numbers")
        return int(lo), int(hi), int(cov)

    def _export(self, t, region, min_coverage):
        """agx_unit_unitigs, or agx_unit_unitigs_region when a window or a threshold is given (region alone: the unit's own coverage; min_coverage alone: every position)."""
        if region is None and min_coverage is None:
            self._check(lib().agx_unit_unitigs(self._h, ctypes.byref(t)))
            return
        self._check(lib().agx_unit_unitigs_region(self._h, *self._window(region, min_coverage), ctypes.byref(t)))

    def edge_support(self):
        """How many events name each edge of the built graph (agx_unit_edge_support; the unit was created with edge_support=True): edge_start and edge_dst are graph()'s,
        edge_cnt[e] the support of edge e, n_events the events counted and n_contributions the sum of edge_cnt.  The first call after a build counts on the device; later
        calls reuse the counters."""
        s = EdgeSupport()
        self._check(lib().agx_unit_edge_support(self._h, ctypes.byref(s)))
        try:
            return {"n_nodes": s.n_nodes, "n_edges": s.n_edges, "n_events": s.n_events, "n_contributions": s.n_contributions,
                    "edge_start": _arr(s.edge_start, s.n_nodes + 1, "uint32"), "edge_dst": _arr(s.edge_dst, s.n_edges, "uint32"), "edge_cnt": _arr(s.edge_cnt, s.n_edges, "uint32")}
        finally:
            lib().agx_edge_support_free(ctypes.byref(s))

    def edge_reads(self, region=None, max_support=None):
        """The hits behind the edges of a window (agx_unit_edge_reads; the unit was created with keep_counts=True and edge_support=True): every edge whose source position
        lies in region = (lo, hi) (None: every position) and whose support is <= max_support (None: every edge), as src_pos, src_var, dst_pos, dst_var, support per edge in
        the order (src_pos, src_var, dst_pos, dst_var), and the hit numbers of the events that name edge e, ascending, in hit[hit_off[e]:hit_off[e + 1]].  A hit number is
        the hit's place in file order: the index into front()["dhit"] after undoing perm, the i-th hit handed to push_pairs."""
        lo, hi = region if region is not None else (0, self.stats()["n_pos"])
        top = 0xFFFFFFFF if max_support is None else max_support
        for v in (lo, hi, top):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise AgxError(AGX_E_ARG, "edge reads: region bounds and max_support are unsigned 32-bit numbers")
        r = EdgeReads()
        self._check(lib().agx_unit_edge_reads(self._h, int(lo), int(hi), int(top), ctypes.byref(r)))
        try:
            out = {k: _arr(getattr(r, k), r.n_edges, "uint32") for k in EDGE_READS_EDGE}
            out.update(hit_off=_arr(r.hit_off, r.n_edges + 1, "uint64"), hit=_arr(r.hit, r.n_hits, "uint32"))
            return out
        finally:
            lib().agx_edge_reads_free(ctypes.byref(r))

    def _export_support(self, t, region, min_coverage, m=None):
        """agx_unit_unitigs_support over the window and threshold of _window(); returns the links' support as a ctypes array the caller frees (agx_link_support_free)."""
        sup = ctypes.POINTER(ctypes.c_uint32)()
        self._check(lib().agx_unit_unitigs_support(self._h, *self._window(region, min_coverage), ctypes.byref(t), ctypes.byref(sup), ctypes.byref(m) if m is not None else None))
        return sup

    def unitigs(self, region=None, min_coverage=None, id_map=False, edge_support=False):
        """The unit's pruned graph compacted into unitigs on the device (agx_unit_unitigs; needs keep_counts): numpy arrays per segment and link, the
        bases as bytes.  region=(lo, hi) and / or min_coverage: the sub-graph of positions [lo, hi) whose nodes are alive at that coverage
        (agx_unit_unitigs_region), at a cost that follows the window.  id_map=True (needs keep_paths; agx_unit_unitigs_mapped): the same table of the window
        (every position without a region) at the threshold (the unit's coverage without one) with one more entry, "id_map": the runs of walk ids whose nodes
        are in the export (id_first, id_last, seg, rank_first) and the unit's n_pos and n_ids."""
        if edge_support:
            return self._unitigs_support(region, min_coverage, id_map)
        t = Unitigs()
        if not id_map:
            self._export(t, region, min_coverage)
            try:
                return _unitigs_arrays(t)
            finally:
                lib().agx_unitigs_free(ctypes.byref(t))
        m = IdMap()
        self._check(lib().agx_unit_unitigs_mapped(self._h, *self._window(region, min_coverage), ctypes.byref(t), ctypes.byref(m)))
        try:
            out = _unitigs_arrays(t)
            out["id_map"] = _idmap_arrays(m)
            return out
        finally:
            lib().agx_unitigs_free(ctypes.byref(t))
            lib().agx_idmap_free(ctypes.byref(m))

    def _unitigs_support(self, region, min_coverage, id_map):
        """unitigs(edge_support=True): the region export's table (every position without a region, the unit's coverage without a threshold) plus "link_support", the
        support of each link's edge (agx_unit_unitigs_support; the unit was created with edge_support=True)."""
        import numpy as np
        t, m = Unitigs(), IdMap() if id_map else None
        sup = self._export_support(t, region, min_coverage, m)
        try:
            out = _unitigs_arrays(t)
            out["link_support"] = np.ctypeslib.as_array(sup, shape=(t.n_links,)).astype("uint32", copy=True) if t.n_links else np.zeros(0, "uint32")
            if id_map:
                out["id_map"] = _idmap_arrays(m)
            return out
        finally:
            lib().agx_unitigs_free(ctypes.byref(t))
            lib().agx_link_support_free(sup)
            if id_map:
                lib().agx_idmap_free(ctypes.byref(m))

    def walk_paths(self):
        """The graph stretches of the records the last finish() wrote to "pre" (agx_unit_walk_paths; needs keep_paths): rec_len, st_off per record, id_first, id_last,
        base_off, joined per stretch, as numpy arrays."""
        w = WalkPaths()
        self._check(lib().agx_unit_walk_paths(self._h, ctypes.byref(w)))
        try:
            nr, ns = w.n_recs, w.n_stretches
            return {"rec_len": _arr(w.rec_len, nr, "uint64"), "st_off": _arr(w.st_off, nr + 1, "uint64"), "id_first": _arr(w.id_first, ns, "uint32"),
                    "id_last": _arr(w.id_last, ns, "uint32"), "base_off": _arr(w.base_off, ns, "uint64"), "joined": _arr(w.joined, ns, "uint8")}
        finally:
            lib().agx_walk_paths_free(ctypes.byref(w))

    def walk_evidence(self, w=None, min_depth=0, min_support=0, tracks=False, records=None):
        """The evidence under the records of a stretch table (agx_unit_walk_evidence; needs keep_counts, and edge_support for the steps): w is a dict like walk_paths()
        returns (None: walk_paths() itself).  Per record rec_graph_bases, rec_steps, rec_depth_sum, rec_depth_min / _at, rec_step_min / _at; the weak intervals at the
        thresholds iv_rec, iv_first, iv_last, iv_depth_min, iv_step_min; the totals n_graph_bases, n_steps, n_steps_without_edge.  0xFFFFFFFF: no number.  tracks=True:
        also depth, votes and step per graph base of the records `records` = (lo, hi) (None: all) with track_off per stretch of those records, and rec_lo, rec_hi."""
        return self._under_records(w, (min_depth, min_support), tracks, records, "walk evidence: thresholds and record bounds are unsigned 32-bit numbers", WalkEvidence, "walk_evidence",
                                   ("n_graph_bases", "n_steps", "n_steps_without_edge"), REC_EVIDENCE, IV_EVIDENCE, ("depth", "votes", "step"))

    def _under_records(self, w, thresholds, tracks, records, bad, struct, call, totals, rec_names, iv_names, track_names):
        """walk_evidence and walk_span: the stretch table as a struct, the 32-bit checks (bad: the message), agx_unit_<call> into a `struct`, and its totals, per-record
        arrays (the first three 64-bit), intervals and tracks, by their names, as the dict the two return."""
        import numpy as np
        if w is None:
            w = self.walk_paths()
        ws, _keep = _walk_paths_struct(w)
        lo, hi = (0, ws.n_recs) if records is None else records
        for v in thresholds + (lo, hi):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise AgxError(AGX_E_ARG, bad)
        e = struct()
        self._check(getattr(lib(), "agx_unit_" + call)(self._h, ctypes.byref(ws), *(int(v) for v in thresholds), 1 if tracks else 0, int(lo), int(hi), ctypes.byref(e)))
        try:
            out = {k: getattr(e, k) for k in totals}
            for k in rec_names:
                out[k] = _arr(getattr(e, k), e.n_recs, "uint64" if k in rec_names[:3] else "uint32")
            for k in iv_names:
                out[k] = _arr(getattr(e, k), e.n_intervals, "uint32")
            if tracks:
                st = np.asarray(w["st_off"]).astype(np.int64)
                n_st = int(st[hi] - st[lo]) if len(st) else 0
                out.update(rec_lo=e.rec_lo, rec_hi=e.rec_hi, track_off=_arr(e.track_off, n_st + 1, "uint64"))
                for k in track_names:
                    out[k] = _arr(getattr(e, k), e.n_track, "uint32")
            return out
        finally:
            getattr(lib(), "agx_" + call + "_free")(ctypes.byref(e))

    def pair_span(self, region=None):
        """The read pairs across each position (agx_unit_pair_span; needs keep_counts, before download(), trim() and release()): for region = (lo, hi) (None: every
        position) span[x - lo], the fragments of kept hits that cover position x, and cross[x - lo], those that cover x and x + 1; n_kept, n_outside (the unit's kept
        hits, and those of them that lie beyond its positions) and n_fragments (the fragments that meet the region); pos_lo, pos_hi."""
        lo, hi = region if region is not None else (0, self.stats()["n_pos"])
        for v in (lo, hi):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise AgxError(AGX_E_ARG, "pair span: region bounds are unsigned 32-bit numbers")
        s = PairSpan()
        self._check(lib().agx_unit_pair_span(self._h, int(lo), int(hi), ctypes.byref(s)))
        try:
            n = s.pos_hi - s.pos_lo
            return {"pos_lo": s.pos_lo, "pos_hi": s.pos_hi, "n_kept": s.n_kept, "n_fragments": s.n_fragments, "n_outside": s.n_outside, "span": _arr(s.span, n, "uint32"), "cross": _arr(s.cross, n, "uint32")}
        finally:
            lib().agx_pair_span_free(ctypes.byref(s))

    def walk_span(self, w=None, min_span=0, tracks=False, records=None):
        """The pair span under the records of a stretch table (agx_unit_walk_span; needs keep_counts): w is a dict like walk_paths() returns (None: walk_paths() itself).
        Per record rec_graph_bases, rec_steps, rec_span_sum, rec_span_min / _at, rec_step_min / _at; the thin intervals at min_span iv_rec, iv_first, iv_last,
        iv_span_min, iv_step_min; the totals n_graph_bases, n_steps, n_jump_steps, n_steps_not_forward.  0xFFFFFFFF: no number.  tracks=True: also pos, span and step per
        graph base of the records `records` = (lo, hi) (None: all) with track_off per stretch of those records, and rec_lo, rec_hi."""
        return self._under_records(w, (min_span,), tracks, records, "walk span: the threshold and record bounds are unsigned 32-bit numbers", WalkSpan, "walk_span",
                                   ("n_graph_bases", "n_steps", "n_jump_steps", "n_steps_not_forward"), REC_SPAN, IV_SPAN, ("pos", "span", "step"))

    def mate_links(self, w=None, min_pairs=1):
        """The read pairs that join two records of a stretch table (agx_unit_mate_links; needs keep_counts): w is a dict like walk_paths() returns (None: walk_paths()
        itself).  The totals n_kept, n_outside, n_fragments, n_unowned, n_inside, n_open, n_link_pairs, n_links_all, n_owned, n_shadowed; per record rec_inside,
        rec_open_left, rec_open_right, rec_links_out, rec_links_in; per link with n_pairs >= min_pairs, by (a, b): a, b, n_pairs, len_sum, lo_min, lo_max, hi_min, hi_max;
        n_passes and n_slots: the passes over the hits the call took and the slots of its table; ms: the call's host wall time."""
        if w is None:
            w = self.walk_paths()
        ws, _keep = _walk_paths_struct(w)
        if not 0 <= int(min_pairs) <= 0xFFFFFFFF:
            raise AgxError(AGX_E_ARG, "mate links: the threshold is an unsigned 32-bit number")
        l = MateLinks()
        self._check(lib().agx_unit_mate_links(self._h, ctypes.byref(ws), int(min_pairs), ctypes.byref(l)))
        try:
            out = {k: int(getattr(l, k)) for k in TOTALS_LINKS}
            out["ms"] = float(l.ms)
            for k in REC_LINKS:
                out[k] = _arr(getattr(l, k), l.n_recs, "uint32")
            for k in LINK_LINKS:
                out[k] = _arr(getattr(l, k), l.n_links, "uint64" if k == "len_sum" else "uint32")
            return out
        finally:
            lib().agx_mate_links_free(ctypes.byref(l))

    def bubbles(self, region=None, min_coverage=None, max_nodes=None, edge_support=False):
        """The variant sites of the unit's graph, found on the device (agx_unit_bubbles; needs keep_counts): the forks of the graph unitigs(region, min_coverage) gives,
        counted by class — n_forks, n_bubbles_all, n_tip, n_nested, n_sinks_differ, n_sink_shared, longest_branch, with n_segs and n_links —, and the table of the bubbles
        whose branch segments have max_nodes nodes at most (None: all), by source segment: src_pos, src_var, src_last, sink_pos, sink_var, br_off per bubble (one offset
        more); br_pos, br_var (0xFFFFFFFF: a direct branch), br_nodes, br_cov, br_seq_off (one offset more) per branch row; seq, the branch segments' bases, as bytes.
        edge_support=True (the unit was created with edge_support=True): also br_sup_in, br_sup_out.  ms and bytes_down: the call's host wall time and download."""
        mx = 0xFFFFFFFF if max_nodes is None else int(max_nodes)
        if not 0 <= mx <= 0xFFFFFFFF:
            raise AgxError(AGX_E_ARG, "bubbles: max_nodes is an unsigned 32-bit number")
        b = Bubbles()
        self._check(lib().agx_unit_bubbles(self._h, *self._window(region, min_coverage), mx, 1 if edge_support else 0, ctypes.byref(b)))
        try:
            return _bubbles_arrays(b)
        finally:
            lib().agx_bubbles_free(ctypes.byref(b))

    def gfa(self, unit=0, region=None, min_coverage=None, edge_support=False):
        """GFA 1.0 S and L lines of the unit's unitigs, segments named u<unit>_<pos>_<var> (no header line); region and min_coverage as in unitigs().
        edge_support=True: every L line also carries RC:i:<events that name the link's edge> (agx_unitigs_gfa_support)."""
        t = Unitigs()
        if edge_support:
            sup = self._export_support(t, region, min_coverage)
            try:
                return _gfa_text(t, unit, sup)
            finally:
                lib().agx_unitigs_free(ctypes.byref(t))
                lib().agx_link_support_free(sup)
        self._export(t, region, min_coverage)
        try:
            return _gfa_text(t, unit)
        finally:
            lib().agx_unitigs_free(ctypes.byref(t))


def _unitigs_arrays(t):
    import numpy as np

    ns, nl = t.n_segs, t.n_links
    return {"head_pos": _arr(t.head_pos, ns, "uint32"), "head_var": _arr(t.head_var, ns, "uint32"), "n_nodes": _arr(t.n_nodes, ns, "uint32"),
            "last_pos": _arr(t.last_pos, ns, "uint32"), "coverage": _arr(t.coverage, ns, "uint64"),
            "seq_off": _arr(t.seq_off, ns + 1, "uint64") if ns else np.zeros(1, "uint64"),
            "seq": ctypes.string_at(t.seq, t.n_bases) if t.seq and t.n_bases else b"",
            "link_from": _arr(t.link_from, nl, "uint32"), "link_to": _arr(t.link_to, nl, "uint32")}


def _idmap_arrays(m):
    n = m.n_runs
    return {"n_pos": m.n_pos, "n_ids": m.n_ids, "id_first": _arr(m.id_first, n, "uint32"), "id_last": _arr(m.id_last, n, "uint32"), "seg": _arr(m.seg, n, "uint32"), "rank_first": _arr(m.rank_first, n, "uint32")}


def gfa_paths(t, w, unit=0):
    """GFA P lines (no header) that lay the records of w (the dict Unit.walk_paths() returns) over the segments of t (the dict Unit.unitigs(id_map=True) returns):
    agx_unitigs_paths_gfa; host only, needs no device."""
    import numpy as np
    ts, _keep = _unitigs_struct(t)
    im = t["id_map"]
    mk = {k: np.ascontiguousarray(im[k], dtype="uint32") for k in ("id_first", "id_last", "seg", "rank_first")}
    m = IdMap()
    m.n_runs, m.n_pos, m.n_ids = len(mk["id_first"]), int(im["n_pos"]), int(im["n_ids"])
    for k, a in mk.items():
        setattr(m, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    ws, _keep_w = _walk_paths_struct(w)
    return _text(lib().agx_unitigs_paths_gfa, ctypes.byref(ts), ctypes.byref(m), ctypes.byref(ws), unit, what="agx_unitigs_paths_gfa: the unitig table, the id map and the stretches do not agree")


def _walk_paths_struct(w):
    """An agx_walk_paths over the arrays of a dict like Unit.walk_paths() returns; returns (struct, the buffers it points into)."""
    import numpy as np
    wk = {k: np.ascontiguousarray(w[k], dtype=dt) for k, dt in (("rec_len", "uint64"), ("st_off", "uint64"), ("id_first", "uint32"), ("id_last", "uint32"),
                                                                 ("base_off", "uint64"), ("joined", "uint8"))}
    ws = WalkPaths()
    ws.n_recs, ws.n_stretches = len(wk["rec_len"]), len(wk["id_first"])
    for k, a in wk.items():
        setattr(ws, k, a.ctypes.data_as(ctypes.POINTER({"uint64": ctypes.c_uint64, "uint32": ctypes.c_uint32, "uint8": ctypes.c_uint8}[a.dtype.name])))
    return ws, wk


def evidence_bed(e, unit=0):
    """BED text of the weak intervals of a dict like Unit.walk_evidence() returns (agx_walk_evidence_bed; host only, needs no device)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(e[k], dtype="uint32") for k in IV_EVIDENCE}
    s = WalkEvidence()
    s.n_recs, s.n_intervals = len(e["rec_graph_bases"]), len(keep["iv_rec"])
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return _text(lib().agx_walk_evidence_bed, ctypes.byref(s), unit, what="agx_walk_evidence_bed: the interval table is inconsistent")


def edge_reads_tsv(r, unit=0):
    """TSV text of a dict like Unit.edge_reads() returns, one line per edge: unit, src_pos, src_var, dst_pos, dst_var, support, the hit numbers joined by commas
    (agx_edge_reads_tsv; host only, needs no device)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(r[k], dtype="uint32") for k in EDGE_READS_EDGE + ("hit",)}
    keep["hit_off"] = np.ascontiguousarray(r["hit_off"], dtype="uint64")
    s = EdgeReads()
    s.n_edges, s.n_hits = len(keep["src_pos"]), len(keep["hit"])
    if len(keep["hit_off"]) != s.n_edges + 1 or any(len(keep[k]) != s.n_edges for k in EDGE_READS_EDGE):
        raise AgxError(AGX_E_ARG, "agx_edge_reads_tsv: one entry per edge, and one offset more")
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64 if k == "hit_off" else ctypes.c_uint32)))
    return _text(lib().agx_edge_reads_tsv, ctypes.byref(s), unit, what="agx_edge_reads_tsv: the table is inconsistent")


def span_bed(e, unit=0):
    """BED text of the thin intervals of a dict like Unit.walk_span() returns (agx_walk_span_bed; host only, needs no device)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(e[k], dtype="uint32") for k in IV_SPAN}
    s = WalkSpan()
    s.n_recs, s.n_intervals = len(e["rec_graph_bases"]), len(keep["iv_rec"])
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    return _text(lib().agx_walk_span_bed, ctypes.byref(s), unit, what="agx_walk_span_bed: the interval table is inconsistent")


def links_tsv(l, unit=0):
    """Text of the links of a dict like Unit.mate_links() returns, one line per link (agx_mate_links_tsv; host only, needs no device)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(l[k], dtype="uint64" if k == "len_sum" else "uint32") for k in LINK_LINKS}
    s = MateLinks()
    s.n_recs, s.n_links = len(l["rec_inside"]), len(keep["a"])
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64 if k == "len_sum" else ctypes.c_uint32)))
    return _text(lib().agx_mate_links_tsv, ctypes.byref(s), unit, what="agx_mate_links_tsv: the link table is inconsistent")


def _bubbles_arrays(b):
    out = {k: int(getattr(b, k)) for k in TOTALS_BUBBLES}
    out.update(ms=float(b.ms), bytes_down=int(b.bytes_down), has_support=bool(b.has_support))
    for k in BUBBLE_BUBBLES:
        out[k] = _arr(getattr(b, k), b.n_bubbles, "uint32")
    out["br_off"] = _arr(b.br_off, b.n_bubbles + 1, "uint32")
    for k in BRANCH_BUBBLES:
        out[k] = _arr(getattr(b, k), b.n_branches, "uint64" if k == "br_cov" else "uint32")
    out["br_seq_off"] = _arr(b.br_seq_off, b.n_branches + 1, "uint64")
    if b.has_support:
        out["br_sup_in"], out["br_sup_out"] = _arr(b.br_sup_in, b.n_branches, "uint32"), _arr(b.br_sup_out, b.n_branches, "uint32")
    out["seq"] = ctypes.string_at(b.seq, b.n_bases) if b.seq and b.n_bases else b""
    return out


def unitigs_bubbles(t, link_support=None, max_nodes=None):
    """The bubbles of a unitig table given as the dict Unit.unitigs() returns, as Unit.bubbles() gives them for the same graph (agx_unitigs_bubbles; host only, needs no
    device).  link_support: one number per link (Unit.unitigs(edge_support=True)["link_support"]) for br_sup_in and br_sup_out, or None."""
    import numpy as np
    ts, _keep = _unitigs_struct(t)
    sup = None
    if link_support is not None:
        sup = np.ascontiguousarray(link_support, dtype="uint32")
        if len(sup) != ts.n_links:
            raise AgxError(AGX_E_ARG, "agx_unitigs_bubbles: one number per link")
        sup = np.concatenate([sup, np.zeros(1, "uint32")])      # (never a null pointer, also without links)
    mx = 0xFFFFFFFF if max_nodes is None else int(max_nodes)
    if not 0 <= mx <= 0xFFFFFFFF:
        raise AgxError(AGX_E_ARG, "agx_unitigs_bubbles: max_nodes is an unsigned 32-bit number")
    b = Bubbles()
    rc = lib().agx_unitigs_bubbles(ctypes.byref(ts), sup.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if sup is not None else None, mx, ctypes.byref(b))
    if rc != AGX_OK:
        raise AgxError(rc, "agx_unitigs_bubbles: the unitig table is inconsistent")
    try:
        return _bubbles_arrays(b)
    finally:
        lib().agx_bubbles_free(ctypes.byref(b))


def bubbles_tsv(b, unit=0):
    """Text of the bubbles of a dict like Unit.bubbles() returns, one line per bubble (agx_bubbles_tsv; host only, needs no device)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(b[k], dtype="uint32") for k in BUBBLE_BUBBLES + ("br_off", "br_pos", "br_var", "br_nodes")}
    keep.update({k: np.ascontiguousarray(b[k], dtype="uint64") for k in ("br_cov", "br_seq_off")})
    sup = "br_sup_in" in b and b["br_sup_in"] is not None
    if sup:
        keep.update({k: np.concatenate([np.ascontiguousarray(b[k], dtype="uint32"), np.zeros(1, "uint32")]) for k in ("br_sup_in", "br_sup_out")})
    seq = ctypes.create_string_buffer(bytes(b["seq"]), max(1, len(b["seq"])))
    s = Bubbles()
    s.n_bubbles, s.n_branches, s.n_bases, s.has_support = len(keep["src_pos"]), len(keep["br_pos"]), len(b["seq"]), 1 if sup else 0
    if len(keep["br_off"]) != s.n_bubbles + 1 or len(keep["br_seq_off"]) != s.n_branches + 1 or any(len(keep[k]) != s.n_bubbles for k in BUBBLE_BUBBLES) or \
            any(len(keep[k]) != s.n_branches for k in BRANCH_BUBBLES) or (sup and any(len(keep[k]) != s.n_branches + 1 for k in ("br_sup_in", "br_sup_out"))):
        raise AgxError(AGX_E_ARG, "agx_bubbles_tsv: one entry per bubble and per branch row, and one offset more")
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64 if a.dtype == np.uint64 else ctypes.c_uint32)))
    s.seq = ctypes.cast(seq, ctypes.c_void_p).value
    return _text(lib().agx_bubbles_tsv, ctypes.byref(s), unit, what="agx_bubbles_tsv: the bubble table is inconsistent")


def _gfa_text(t, unit, link_support=None):
    """link_support: a ctypes uint32 pointer for the RC tags (agx_unitigs_gfa_support), or None"""
    what = "agx_unitigs_gfa: the unitig table is inconsistent"
    if link_support is None:
        return _text(lib().agx_unitigs_gfa, ctypes.byref(t), unit, what=what)
    return _text(lib().agx_unitigs_gfa_support, ctypes.byref(t), link_support, unit, what=what)


def _unitigs_struct(u):
    """An agx_unitigs over the arrays of a dict like Unit.unitigs() returns; returns (struct, the buffers it points into)."""
    import numpy as np
    keep = {k: np.ascontiguousarray(u[k], dtype=dt) for k, dt in (("head_pos", "uint32"), ("head_var", "uint32"), ("n_nodes", "uint32"), ("last_pos", "uint32"),
                                                                   ("coverage", "uint64"), ("seq_off", "uint64"), ("link_from", "uint32"), ("link_to", "uint32"))}
    seq = ctypes.create_string_buffer(bytes(u["seq"]), max(1, len(u["seq"])))
    t = Unitigs()
    t.n_segs, t.n_links, t.n_bases = len(keep["head_pos"]), len(keep["link_from"]), len(u["seq"])
    for k, a in keep.items():
        setattr(t, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64 if a.dtype == np.uint64 else ctypes.c_uint32)))
    t.seq = ctypes.cast(seq, ctypes.c_void_p).value
    return t, (keep, seq)


def unitigs_gfa(u, unit=0, edge_support=False):
    """GFA S/L lines (no header) of a unitig table given as the dict Unit.unitigs() returns (agx_unitigs_gfa; host only, needs no device).  edge_support=True: with the RC
    tags of u["link_support"] (agx_unitigs_gfa_support)."""
    import numpy as np
    t, _keep = _unitigs_struct(u)
    if not edge_support:
        return _gfa_text(t, unit)
    sup = np.ascontiguousarray(u["link_support"], dtype="uint32")
    if len(sup) != t.n_links:
        raise AgxError(AGX_E_ARG, "agx_unitigs_gfa_support: one number per link")
    return _gfa_text(t, unit, sup.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))


def cache_build(tmp_dir, unit, batch=0, device=0, reads=None, k=5):
    """Writes tmp_dir/_agx_unit.<unit>.bin (the unit's staged arrays) from the five text files; load_files then takes it instead of the text
    (units of the same k and batch size only)."""
    p = Params(k, 50, 20, batch, device, 0)
    err = ctypes.create_string_buffer(512)
    rc = lib().agx_unit_cache_build(ctypes.byref(p), tmp_dir.encode(), unit, reads._h if reads is not None else None, err, 512)
    if rc != AGX_OK:
        raise AgxError(rc, err.value.decode(errors="replace"))


def run_unit(tmp_dir, unit, k=5, insert_variation=50, coverage=20, batch=0, device=0, write_files=False):
    """The five-call seam in one call (agx_run_unit)."""
    p = Params(k, insert_variation, coverage, batch, device, 0)
    r = Result()
    err = ctypes.create_string_buffer(512)
    rc = lib().agx_run_unit(ctypes.byref(p), tmp_dir.encode(), unit, 1 if write_files else 0, ctypes.byref(r), err, 512)
    if rc != AGX_OK:
        raise AgxError(rc, err.value.decode(errors="replace"))
    return _take(r)


def usable_cpus():
    """CPUs this process can keep busy: its affinity mask capped by the CPU quota of its control group (cgroup v2 cpu.max) — what the loaders size
    their thread teams by (agx_host.cpp: usable_cpus)."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max" and int(period) > 0:
            n = max(1, min(n, -(-int(quota) // int(period))))
    except Exception:
        pass
    return n
