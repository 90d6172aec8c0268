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

struct Out {  // an output array the caller gave: where it lies in the staging buffer
    void *user;
    size_t bytes;
    size_t off = 0;
};

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
        char *const wsp = h->asm_scratch;

        GraphParams p{};
        asm_bind(p.a, h, in, b, staged, ws);
        uint32_t *const kc = (uint32_t *)(wsp + w_kc.off);
        p.a.flags = W.dev_ptr(o_fl);
        p.a.n_sequences = kc;
        p.a.n_non_unique = kc + n_graphs;
        p.a.n_tracked = kc + 2 * n_graphs;
        p.a.n_distinct = kc + 3 * n_graphs;
        p.a.ref_flags = (uint8_t *)(wsp + w_ff.off);
        p.a.read_flags = (uint8_t *)(wsp + w_df.off);
        p.a.want_ids = false;
        p.num_pruning_samples = num_pruning_samples;
        p.read_sample = W.dev_ptr(s_sm);
        p.region_n_samples = W.dev_ptr(s_ns);
        p.read_rank = (uint32_t *)(wsp + w_rk.off);
        p.read_group = (uint32_t *)(wsp + w_rg.off);
        p.order = (uint32_t *)(wsp + w_or.off);
        p.n_yield = (uint32_t *)(wsp + w_ny.off);
        p.n_groups = (uint32_t *)(wsp + w_ng.off);
        p.ref_handle = (uint32_t *)(wsp + w_fh.off);
        p.read_handle = (uint32_t *)(wsp + w_dh.off);
        p.ref_edge = (uint32_t *)(wsp + w_fe.off);
        p.read_edge = (uint32_t *)(wsp + w_de.off);
        p.trie_claim = (unsigned long long *)(wsp + w_tc.off);
        p.v_stamp = (unsigned long long *)(wsp + w_vs.off);
        p.v_in1 = (unsigned long long *)(wsp + w_v1.off);
        p.v_in2 = (unsigned long long *)(wsp + w_v2.off);
        p.v_inedge = (uint32_t *)(wsp + w_ve.off);
        p.v_index = (uint32_t *)(wsp + w_vi.off);
        p.e_key = (unsigned long long *)(wsp + w_ek.off);
        p.e_stamp = (unsigned long long *)(wsp + w_es.off);
        p.e_index = (uint32_t *)(wsp + w_ei.off);
        p.seq_n_vertices = (uint32_t *)(wsp + w_sv.off);
        p.seq_n_edges = (uint32_t *)(wsp + w_se.off);
        p.seq_vertex_base = (uint32_t *)(wsp + w_bv.off);
        p.seq_edge_base = (uint32_t *)(wsp + w_be.off);
        p.n_vertices = W.dev_ptr(o_nv);
        p.n_edges = W.dev_ptr(o_ne);
        p.n_ref_path = W.dev_ptr(o_np);

        if (!hip_ok(h, hipMemcpyAsync(W.dev, W.host, L.in_bytes, hipMemcpyHostToDevice, S), "H2D assembly graph") ||
            !hip_ok(h, launch_graph_build(p, S), "assembly graph kernels, first half") ||
            !hip_ok(h, hipMemcpyAsync(W.host + L.out_begin, W.dev + L.out_begin, L.total - L.out_begin, hipMemcpyDeviceToHost, S), "D2H assembly graph sizes") ||
            !hip_ok(h, hipStreamSynchronize(S), "sync(assembly graph sizes)"))
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
        Out outs[11] = {{vertex_seq, 4 * (size_t)V}, {vertex_pos, 4 * (size_t)V}, {vertex_flags, V}, {edge_src, 4 * (size_t)E}, {edge_dst, 4 * (size_t)E},
                        {edge_is_ref, E}, {edge_multiplicity, 4 * (size_t)E}, {edge_pruning_multiplicity, 4 * (size_t)E}, {ref_path, 4 * (size_t)P},
                        {ref_vertex, planes ? 4 * nk * n_ref_bases : 0}, {read_vertex, planes ? 4 * nk * n_read_bases : 0}};
        bool any = false;
        for (Out &o : outs) {
            o.off = M.out<char>(o.bytes).off;
            any |= o.bytes != 0;
        }
        if (any) {
            if (!G.reserve(h, M, "assembly graph outputs")) return PHMM_ERR_HIP;
            h->stat_staged_bytes += M.in_bytes;
            auto out_ptr = [&](int i) -> void * { return outs[i].bytes ? G.dev + outs[i].off : nullptr; };
            p.vertex_off = G.dev_ptr(s_vo);
            p.edge_off = G.dev_ptr(s_eo);
            p.ref_path_off = G.dev_ptr(s_po);
            p.count_off = G.dev_ptr(s_co);
            p.count_width = G.dev_ptr(s_cw);
            p.counts = G.dev_ptr(w_ct);
            p.edge_group = G.dev_ptr(w_eg);
            p.n_counts = n_counts;
            p.max_edges = max_edges;
            p.vertex_seq = (uint32_t *)out_ptr(0);
            p.vertex_pos = (uint32_t *)out_ptr(1);
            p.vertex_flags = (uint8_t *)out_ptr(2);
            p.edge_src = (uint32_t *)out_ptr(3);
            p.edge_dst = (uint32_t *)out_ptr(4);
            p.edge_is_ref = (uint8_t *)out_ptr(5);
            p.edge_multiplicity = (uint32_t *)out_ptr(6);
            p.edge_pruning_multiplicity = (uint32_t *)out_ptr(7);
            p.ref_path = (uint32_t *)out_ptr(8);
            p.ref_vertex = planes ? (uint32_t *)out_ptr(9) : nullptr;
            p.read_vertex = planes ? (uint32_t *)out_ptr(10) : nullptr;
            p.want_planes = planes;
            if (!hip_ok(h, hipMemcpyAsync(G.dev, G.host, M.in_bytes, hipMemcpyHostToDevice, S), "H2D assembly graph offsets") ||
                !hip_ok(h, launch_graph_fill(p, S), "assembly graph kernels, second half") ||
                !hip_ok(h, hipMemcpyAsync(G.host + M.out_begin, G.dev + M.out_begin, M.total - M.out_begin, hipMemcpyDeviceToHost, S), "D2H assembly graph") ||
                !hip_ok(h, hipStreamSynchronize(S), "sync(assembly graph)"))
                return PHMM_ERR_HIP;
            for (const Out &o : outs)
                if (o.bytes) memcpy(o.user, G.host + o.off, o.bytes);
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
