// phmm_assembly_graph (include/phmm.h): host side -- validation, staging and the two halves of the call.  The first half runs
// the k-mer stage and sizes every graph on the device; the host reads the sizes, lays the outputs out and checks the
// capacities; the second half fills them.  Every step runs on the device (phmm_graph_kernels.hip); there is no CPU path here.
#include <cstring>
#include <string>
#include <vector>

#include "phmm_asm_host.hpp"
#include "phmm_graph_internal.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_graph: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int phmm_assembly_graph(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                                   const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases,
                                   const uint8_t *read_quals, const uint32_t *read_first, const uint32_t *read_len,
                                   const uint32_t *read_sample, uint32_t n_k, const uint32_t *k, uint32_t min_base_quality,
                                   uint32_t num_pruning_samples, const uint32_t *capacity, uint32_t *required, uint32_t *flags,
                                   uint32_t *n_vertices, uint32_t *n_edges, uint32_t *n_ref_path, uint32_t *vertex_off,
                                   uint32_t *edge_off, uint32_t *ref_path_off, uint32_t *vertex_seq, uint32_t *vertex_pos,
                                   uint8_t *vertex_flags, uint32_t *edge_src, uint32_t *edge_dst, uint8_t *edge_is_ref,
                                   uint32_t *edge_multiplicity, uint32_t *edge_pruning_multiplicity, uint32_t *ref_path,
                                   uint32_t *ref_vertex, uint32_t *read_vertex) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (num_pruning_samples < 1 || num_pruning_samples > PHMM_GRAPH_MAX_PRUNING_SAMPLES)
            return fail(h, "num_pruning_samples is " + std::to_string(num_pruning_samples) + ", outside 1.." + std::to_string(PHMM_GRAPH_MAX_PRUNING_SAMPLES));
        if (!capacity || !required) return fail(h, "a required pointer is NULL (capacity, required)");
        if ((capacity[0] && (!vertex_seq || !vertex_pos || !vertex_flags)) ||
            (capacity[1] && (!edge_src || !edge_dst || !edge_is_ref || !edge_multiplicity || !edge_pruning_multiplicity)) || (capacity[2] && !ref_path))
            return fail(h, "an offsets array has a capacity and no data (vertex, edge or ref_path arrays)");
        const AsmInputs in{n_regions, region_ref_off, ref_bases, region_read_off, read_off, read_bases, read_quals, read_first, read_len, n_k, k, min_base_quality};
        const AsmOutputsGiven given{!ref_vertex == !read_vertex, "ref_vertex and read_vertex are given together or not at all",
                                    flags && n_vertices && n_edges && n_ref_path && vertex_off && edge_off && ref_path_off, true, "ref_bases", true,
                                    "read_bases, read_quals"};
        AsmBatch b;
        if (const int rc = asm_check(h, "phmm_assembly_graph", in, given, b)) return rc;
        if (!b.n_regions) {
            required[0] = required[1] = required[2] = 0;
            if (vertex_off) vertex_off[0] = 0;
            if (edge_off) edge_off[0] = 0;
            if (ref_path_off) ref_path_off[0] = 0;
            return PHMM_OK;
        }
        const uint32_t n_reads = b.n_reads, n_ref_bases = b.n_ref_bases, n_read_bases = b.n_read_bases;
        // the samples of a region as 0, 1, ... in order of first appearance; NULL is one sample
        std::vector<uint32_t> sample(n_reads, 0), region_n_samples(n_regions, 0);
        for (uint32_t g = 0; g < n_regions; ++g) {
            uint32_t seen[PHMM_GRAPH_MAX_SAMPLES], n = 0;
            for (uint32_t r = region_read_off[g]; r < region_read_off[g + 1]; ++r) {
                const uint32_t v = read_sample ? read_sample[r] : 0;
                uint32_t s = 0;
                while (s < n && seen[s] != v) ++s;
                if (s == n) {
                    if (n == PHMM_GRAPH_MAX_SAMPLES) return fail(h, "region " + std::to_string(g) + ": more than " + std::to_string(PHMM_GRAPH_MAX_SAMPLES) + " samples");
                    seen[n++] = v;
                }
                sample[r] = s;
            }
            region_n_samples[g] = n;
        }
        const bool planes = ref_vertex != nullptr;
        const size_t nk = n_k, n_graphs = nk * n_regions, n_slots = nk * b.n_slots, n_seq = nk * ((size_t)n_regions + n_reads);

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->asm_staging;
        hipStream_t S = h->streams[0];
        // ---- first half: the inputs and the graphs' sizes staged; everything else in the device-only workspace ----------------
        StageLayout L;
        const AsmStaged staged = asm_stage_inputs(L, in, b);
        const auto s_sm = L.in(sample.data(), n_reads), s_ns = L.in(region_n_samples.data(), n_regions);
        L.end_inputs();
        const auto o_fl = L.out<uint32_t>(n_graphs), o_nv = L.out<uint32_t>(n_graphs), o_ne = L.out<uint32_t>(n_graphs), o_np = L.out<uint32_t>(n_graphs);
        StageLayout D;
        const AsmWorkspace ws = asm_plan_workspace(D, b, nk);
        const auto w_kc = D.scratch<uint32_t>(4 * n_graphs);   // the k-mer stage's counts, not reported here
        const auto w_ff = D.scratch<uint8_t>(nk * n_ref_bases), w_df = D.scratch<uint8_t>(nk * n_read_bases);
        const auto w_rk = D.scratch<uint32_t>(nk * n_reads), w_rg = D.scratch<uint32_t>(nk * n_reads), w_or = D.scratch<uint32_t>(nk * n_reads);
        const auto w_ny = D.scratch<uint32_t>(n_graphs), w_ng = D.scratch<uint32_t>(n_graphs);
        const auto w_fh = D.scratch<uint32_t>(nk * n_ref_bases), w_dh = D.scratch<uint32_t>(nk * n_read_bases);
        const auto w_fe = D.scratch<uint32_t>(nk * n_ref_bases), w_de = D.scratch<uint32_t>(nk * n_read_bases);
        const auto w_tc = D.scratch<unsigned long long>(n_slots);
        const auto w_vs = D.scratch<unsigned long long>(2 * n_slots), w_v1 = D.scratch<unsigned long long>(2 * n_slots), w_v2 = D.scratch<unsigned long long>(2 * n_slots);
        const auto w_ve = D.scratch<uint32_t>(2 * n_slots), w_vi = D.scratch<uint32_t>(2 * n_slots);
        const auto w_ek = D.scratch<unsigned long long>(n_slots), w_es = D.scratch<unsigned long long>(n_slots);
        const auto w_ei = D.scratch<uint32_t>(n_slots);
        const auto w_sv = D.scratch<uint32_t>(n_seq), w_se = D.scratch<uint32_t>(n_seq), w_bv = D.scratch<uint32_t>(n_seq), w_be = D.scratch<uint32_t>(n_seq);
        if (!asm_reserve_workspace(h, D)) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "assembly graph staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &wsp = h->asm_scratch;

        GraphParams p{};
        asm_bind(p.a, h, in, b, staged, ws);
        uint32_t *const kc = wsp.ptr(w_kc);
        p.a.flags = W.dev_ptr(o_fl);
        p.a.n_sequences = kc;
        p.a.n_non_unique = kc + n_graphs;
        p.a.n_tracked = kc + 2 * n_graphs;
        p.a.n_distinct = kc + 3 * n_graphs;
        p.a.ref_flags = wsp.ptr(w_ff);
        p.a.read_flags = wsp.ptr(w_df);
        p.a.want_ids = false;
        p.num_pruning_samples = num_pruning_samples;
        p.read_sample = W.dev_ptr(s_sm);
        p.region_n_samples = W.dev_ptr(s_ns);
        p.read_rank = wsp.ptr(w_rk);
        p.read_group = wsp.ptr(w_rg);
        p.order = wsp.ptr(w_or);
        p.n_yield = wsp.ptr(w_ny);
        p.n_groups = wsp.ptr(w_ng);
        p.ref_handle = wsp.ptr(w_fh);
        p.read_handle = wsp.ptr(w_dh);
        p.ref_edge = wsp.ptr(w_fe);
        p.read_edge = wsp.ptr(w_de);
        p.trie_claim = wsp.ptr(w_tc);
        p.v_stamp = wsp.ptr(w_vs);
        p.v_in1 = wsp.ptr(w_v1);
        p.v_in2 = wsp.ptr(w_v2);
        p.v_inedge = wsp.ptr(w_ve);
        p.v_index = wsp.ptr(w_vi);
        p.e_key = wsp.ptr(w_ek);
        p.e_stamp = wsp.ptr(w_es);
        p.e_index = wsp.ptr(w_ei);
        p.seq_n_vertices = wsp.ptr(w_sv);
        p.seq_n_edges = wsp.ptr(w_se);
        p.seq_vertex_base = wsp.ptr(w_bv);
        p.seq_edge_base = wsp.ptr(w_be);
        p.n_vertices = W.dev_ptr(o_nv);
        p.n_edges = W.dev_ptr(o_ne);
        p.n_ref_path = W.dev_ptr(o_np);

        if (!stage_upload(h, W, L, S, "assembly graph sizes") || !hip_ok(h, launch_graph_build(p, S), "assembly graph kernels, first half") ||
            !stage_download(h, W, L, S, "assembly graph sizes"))
            return PHMM_ERR_HIP;

        // ---- the sizes: offsets, capacities ----------------------------------------------------------------------------------------
        const uint32_t *const nv = W.host_ptr(o_nv), *const ne = W.host_ptr(o_ne), *const np = W.host_ptr(o_np);
        std::vector<uint32_t> voff(n_graphs + 1, 0), eoff(n_graphs + 1, 0), poff(n_graphs + 1, 0), width(n_graphs);
        std::vector<unsigned long long> coff(n_graphs);
        unsigned long long n_counts = 0;
        uint32_t max_edges = 0;
        for (size_t o = 0; o < n_graphs; ++o) {   // (a graph's vertices and edges are at most its positions, so the sums fit 32 bits)
            voff[o + 1] = voff[o] + nv[o];
            eoff[o + 1] = eoff[o] + ne[o];
            poff[o + 1] = poff[o] + np[o];
            width[o] = 1 + region_n_samples[o % n_regions];
            coff[o] = n_counts;
            n_counts += (unsigned long long)ne[o] * width[o];
            max_edges = std::max(max_edges, ne[o]);
        }
        const uint32_t V = voff[n_graphs], E = eoff[n_graphs], P = poff[n_graphs];
        const uint32_t need[3] = {V, E, P};
        for (int c = 0; c < 3; ++c)
            if (need[c] > capacity[c]) {
                memcpy(required, need, sizeof need);
                h->err = "phmm_assembly_graph: capacity " + std::to_string(c) + " is " + std::to_string(capacity[c]) + ", " + std::to_string(need[c]) + " needed";
                return h->err_code = PHMM_ERR_EVENT_CAPACITY;
            }

        // ---- second half ----------------------------------------------------------------------------------------------------------
        StagingBuffer &G = h->graph_staging;
        StageLayout M;
        const auto s_vo = M.in(voff.data(), n_graphs + 1), s_eo = M.in(eoff.data(), n_graphs + 1), s_po = M.in(poff.data(), n_graphs + 1);
        const auto s_co = M.in(coff.data(), n_graphs);
        const auto s_cw = M.in(width.data(), n_graphs);
        M.end_inputs();
        const auto w_ct = M.scratch<uint32_t>(n_counts), w_eg = M.scratch<uint32_t>(E);
        const auto o_vq = M.out(vertex_seq, V), o_vp = M.out(vertex_pos, V);
        const auto o_vf = M.out(vertex_flags, V);
        const auto o_es = M.out(edge_src, E), o_ed = M.out(edge_dst, E);
        const auto o_er = M.out(edge_is_ref, E);
        const auto o_em = M.out(edge_multiplicity, E), o_ep = M.out(edge_pruning_multiplicity, E), o_rp = M.out(ref_path, P);
        const auto o_fv = M.out(ref_vertex, planes ? nk * n_ref_bases : 0), o_dv = M.out(read_vertex, planes ? nk * n_read_bases : 0);
        if (M.out_bytes()) {
            if (!G.reserve(h, M, "assembly graph outputs")) return PHMM_ERR_HIP;
            h->stat_staged_bytes += M.in_bytes;
            p.vertex_off = G.dev_ptr(s_vo);
            p.edge_off = G.dev_ptr(s_eo);
            p.ref_path_off = G.dev_ptr(s_po);
            p.count_off = G.dev_ptr(s_co);
            p.count_width = G.dev_ptr(s_cw);
            p.counts = G.dev_ptr(w_ct);
            p.edge_group = G.dev_ptr(w_eg);
            p.n_counts = n_counts;
            p.max_edges = max_edges;
            p.vertex_seq = G.dev_ptr_or_null(o_vq);
            p.vertex_pos = G.dev_ptr_or_null(o_vp);
            p.vertex_flags = G.dev_ptr_or_null(o_vf);
            p.edge_src = G.dev_ptr_or_null(o_es);
            p.edge_dst = G.dev_ptr_or_null(o_ed);
            p.edge_is_ref = G.dev_ptr_or_null(o_er);
            p.edge_multiplicity = G.dev_ptr_or_null(o_em);
            p.edge_pruning_multiplicity = G.dev_ptr_or_null(o_ep);
            p.ref_path = G.dev_ptr_or_null(o_rp);
            p.ref_vertex = G.dev_ptr_or_null(o_fv);
            p.read_vertex = G.dev_ptr_or_null(o_dv);
            p.want_planes = planes;
            if (!stage_round_trip(h, G, M, S, "assembly graph", [&] { return hip_ok(h, launch_graph_fill(p, S), "assembly graph kernels, second half"); }))
                return PHMM_ERR_HIP;
        }
        memcpy(required, need, sizeof need);
        memcpy(flags, W.host_ptr(o_fl), 4 * n_graphs);
        memcpy(n_vertices, nv, 4 * n_graphs);
        memcpy(n_edges, ne, 4 * n_graphs);
        memcpy(n_ref_path, np, 4 * n_graphs);
        memcpy(vertex_off, voff.data(), 4 * (n_graphs + 1));
        memcpy(edge_off, eoff.data(), 4 * (n_graphs + 1));
        memcpy(ref_path_off, poff.data(), 4 * (n_graphs + 1));
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_graph", PHMM_FAIL_CODE)
}
