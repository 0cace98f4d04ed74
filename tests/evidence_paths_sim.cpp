// evidence_paths_sim.cpp — TEST-ONLY: one unit through the serial executor (tests/hostsim/agx_hostsim.cpp, taken in whole: its loaders, simulate() and the graph view it hands
// the host walk) with the walk told to keep the graph stretches of the records it writes (UnitOutput::keep_paths, what AGX_FLAG_KEEP_PATHS sets in the engine).  Gives the
// stretches in the layout of agx_unit_walk_paths and the pre-extended text they belong to.  tests/test_evidence_cases.py compiles this with the executor's other sources into
// a library of its own; the executor's files stay as they are.
#include "hostsim/agx_hostsim.cpp"

extern "C" {

// out: zeroed by the caller, freed with agx_evidence_paths_sim_free; *pre / *pre_len: malloc'd text; 0, or the error's code with its message in err
int agx_evidence_paths_sim(const char *tmp_dir, int unit, int k, int iv, int coverage, long batch, agx_walk_paths *out, char **pre, size_t *pre_len, char *err, size_t err_len) {
    memset(out, 0, sizeof *out); *pre = nullptr; *pre_len = 0;
    try {
        const std::string d = tmp_dir, u = std::to_string(unit);
        Threads T; Pairs P;
        load_unit_reference(d + "/_genome." + u + ".fa", T.ref);
        thread_contigs_from_files(d + "/_contigs.fa", d + "/_contigs_genome." + u + ".psl", T);
        load_pairs_from_files(d + "/_reads.fa", d + "/_reads_genome." + u + ".bowtie", batch, (agx_u32)k, P);
        SimGraph S; int nbig = 0; SimOptions opt; SimRecords R; SimEdges E; SimFront F;
        simulate(T, P, (agx_u32)k, iv, coverage, AGX_MAXV_LDS, S, nbig, opt, R, E, F);
        GraphView G; G.n_pos = (agx_u32)T.ref.size(); G.n_ids = S.n_ids;
        G.meta = S.a_meta.data(); G.str = S.a_str.data(); G.side_xpos = S.side_xpos.data();
        G.sp_bits = S.sp_bits.data(); G.sp_rank = S.sp_rank.data(); G.sp_node = S.sp_node.data(); G.sp_hop = S.sp_hop.data(); G.n_special = S.n_special;
        G.fetch = [](void *ctx, agx_u32 first, agx_u32 stride, agx_u32 rows, agx_u32 width, agx_walknode *o) {
            const SimGraph *g = (const SimGraph *)ctx;
            for (agx_u32 r = 0; r < rows; r++) for (agx_u32 c = 0; c < width; c++) {
                const size_t a = (size_t)first + (size_t)r * stride + c;
                if (a >= g->n_ids) throw Error{E_ARG, "record fetch beyond the walk graph"};
                o[(size_t)r * width + c] = agx_walk_record(g->walk_args, (agx_u32)a);
            }
        };
        G.fetch_ctx = &S;
        G.ovf = S.a_ovf.data(); G.n_ovf = S.ovf.size();
        UnitOutput O; O.keep_paths = true;
        walk_join_scaffold(view_of(T, P), G, O, nullptr);
        auto dup = [](const void *p, size_t bytes) { void *q = malloc(bytes + 8); if (bytes) memcpy(q, p, bytes); return q; };
        const WalkPaths &Q = O.paths; const size_t nr = Q.rec_len.size(), ns = Q.id_first.size();
        out->n_recs = (uint32_t)nr; out->n_stretches = ns;
        out->rec_len = (uint64_t *)dup(Q.rec_len.data(), 8 * nr);
        out->st_off = (uint64_t *)malloc(8 * (nr + 1)); out->st_off[0] = 0; if (nr) memcpy(out->st_off + 1, Q.st_end.data(), 8 * nr);
        out->id_first = (uint32_t *)dup(Q.id_first.data(), 4 * ns); out->id_last = (uint32_t *)dup(Q.id_last.data(), 4 * ns);
        out->base_off = (uint64_t *)dup(Q.base_off.data(), 8 * ns); out->joined = (uint8_t *)dup(Q.joined.data(), ns);
        *pre_len = O.pre_extended.n; *pre = O.pre_extended.release();
        return 0;
    } catch (const Error &e) {
        if (err && err_len) snprintf(err, err_len, "%s", e.msg.c_str());
        return e.code ? e.code : -1;
    }
}

void agx_evidence_paths_sim_free(agx_walk_paths *w, char *pre) {
    free(w->rec_len); free(w->st_off); free(w->id_first); free(w->id_last); free(w->base_off); free(w->joined); free(pre);
    memset(w, 0, sizeof *w);
}

}  // extern "C"
