// phmm_assembly_prune (include/phmm.h): host side -- validation, staging, one launch.  Every step runs on the device
// (phmm_prune_kernels.hip); there is no CPU path here.
#include <cstring>
#include <string>

#include "phmm_prune_internal.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_prune: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int phmm_assembly_prune(phmm_handle *h, uint32_t n_graphs, const uint32_t *vertex_off, const uint32_t *edge_off,
                                   const uint32_t *edge_src, const uint32_t *edge_dst, const uint8_t *edge_is_ref,
                                   const uint32_t *edge_pruning_multiplicity, const uint8_t *vertex_absent, const uint8_t *edge_absent,
                                   uint32_t ops, const uint32_t *prune_factor, uint32_t *graph_flags, uint32_t *n_chains,
                                   uint32_t *n_chains_removed, uint32_t *n_vertices_left, uint32_t *n_edges_left, uint32_t *ref_source,
                                   uint32_t *ref_sink, uint32_t *edge_chain, uint8_t *edge_state, uint8_t *vertex_state) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!ops) return fail(h, "ops is 0: nothing is asked for");
        if (ops & ~(PHMM_PRUNE_OP_CHAINS | PHMM_PRUNE_OP_CONNECT)) return fail(h, "ops has unknown bits (" + std::to_string(ops) + ")");
        if (!vertex_absent != !edge_absent) return fail(h, "vertex_absent and edge_absent are given together or not at all");
        if (!n_graphs) return PHMM_OK;
        if (!vertex_off || !edge_off) return fail(h, "a required pointer is NULL (vertex_off, edge_off)");
        if (!prune_factor) return fail(h, "a required pointer is NULL (prune_factor)");
        if (!graph_flags || !n_chains || !n_chains_removed || !n_vertices_left || !n_edges_left || !ref_source || !ref_sink)
            return fail(h, "a required pointer is NULL (the per-graph outputs)");
        if (vertex_off[0]) return fail(h, "vertex_off does not start at 0");
        if (edge_off[0]) return fail(h, "edge_off does not start at 0");
        for (uint32_t g = 0; g < n_graphs; ++g) {
            if (vertex_off[g + 1] < vertex_off[g]) return fail(h, "graph " + std::to_string(g) + ": vertex_off decreases");
            if (edge_off[g + 1] < edge_off[g]) return fail(h, "graph " + std::to_string(g) + ": edge_off decreases");
        }
        const uint32_t V = vertex_off[n_graphs], E = edge_off[n_graphs];
        if (V && !vertex_state) return fail(h, "a required pointer is NULL (vertex_state)");
        if (E && (!edge_src || !edge_dst || !edge_is_ref || !edge_pruning_multiplicity))
            return fail(h, "a required pointer is NULL (edge_src, edge_dst, edge_is_ref, edge_pruning_multiplicity)");
        if (E && (!edge_chain || !edge_state)) return fail(h, "a required pointer is NULL (edge_chain, edge_state)");
        for (uint32_t g = 0; g < n_graphs; ++g) {
            const uint32_t v0 = vertex_off[g], nv = vertex_off[g + 1] - v0;
            for (uint32_t e = edge_off[g]; e < edge_off[g + 1]; ++e) {
                const auto ed = [&] { return "graph " + std::to_string(g) + ": edge " + std::to_string(e - edge_off[g]) + ": "; };
                if (edge_src[e] >= nv) return fail(h, ed() + "its source " + std::to_string(edge_src[e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (edge_dst[e] >= nv) return fail(h, ed() + "its target " + std::to_string(edge_dst[e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (edge_absent && !edge_absent[e] && (vertex_absent[v0 + edge_src[e]] || vertex_absent[v0 + edge_dst[e]]))
                    return fail(h, ed() + "it is present and an endpoint is absent");
            }
        }

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->prune_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs; the state lies in the device-only workspace ----------------------------------
        StageLayout L;
        const auto s_vo = L.in(vertex_off, (size_t)n_graphs + 1), s_eo = L.in(edge_off, (size_t)n_graphs + 1);
        const auto s_es = L.in(edge_src, E), s_ed = L.in(edge_dst, E);
        const auto s_er = L.in(edge_is_ref, E);
        const auto s_em = L.in(edge_pruning_multiplicity, E);
        const auto s_va = L.in(vertex_absent, vertex_absent ? V : 0), s_ea = L.in(edge_absent, edge_absent ? E : 0);
        const auto s_pf = L.in(prune_factor, n_graphs);
        L.end_inputs();
        const auto o_gf = L.out(graph_flags, n_graphs), o_nc = L.out(n_chains, n_graphs), o_nr = L.out(n_chains_removed, n_graphs);
        const auto o_vl = L.out(n_vertices_left, n_graphs), o_el = L.out(n_edges_left, n_graphs), o_so = L.out(ref_source, n_graphs);
        const auto o_si = L.out(ref_sink, n_graphs), o_ec = L.out(edge_chain, E);
        const auto o_es = L.out(edge_state, E), o_vs = L.out(vertex_state, V);
        StageLayout D;  // the device-only workspace: 20 bytes per vertex, 5 per edge
        const auto w_vi = D.scratch<uint32_t>(V), w_vu = D.scratch<uint32_t>(V), w_ve = D.scratch<uint32_t>(V), w_vr = D.scratch<uint32_t>(V), w_vm = D.scratch<uint32_t>(V);
        const auto w_ep = D.scratch<uint32_t>(E);
        const auto w_eb = D.scratch<uint8_t>(E);
        if (!h->prune_scratch.reserve(h, D, "pruning workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "pruning staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->prune_scratch;

        PruneParams p{};
        p.n_graphs = n_graphs;
        p.ops = ops;
        p.vertex_off = W.dev_ptr(s_vo);
        p.edge_off = W.dev_ptr(s_eo);
        p.edge_src = W.dev_ptr(s_es);
        p.edge_dst = W.dev_ptr(s_ed);
        p.edge_is_ref = W.dev_ptr(s_er);
        p.edge_mult = W.dev_ptr(s_em);
        p.vertex_absent = vertex_absent ? W.dev_ptr(s_va) : nullptr;
        p.edge_absent = edge_absent ? W.dev_ptr(s_ea) : nullptr;
        p.prune_factor = W.dev_ptr(s_pf);
        p.v_in = ws.ptr(w_vi);
        p.v_out = ws.ptr(w_vu);
        p.v_inedge = ws.ptr(w_ve);
        p.v_ref = ws.ptr(w_vr);
        p.v_mark = ws.ptr(w_vm);
        p.e_ptr = ws.ptr(w_ep);
        p.e_bits = ws.ptr(w_eb);
        p.graph_flags = W.dev_ptr_or_null(o_gf);
        p.n_chains = W.dev_ptr_or_null(o_nc);
        p.n_chains_removed = W.dev_ptr_or_null(o_nr);
        p.n_vertices_left = W.dev_ptr_or_null(o_vl);
        p.n_edges_left = W.dev_ptr_or_null(o_el);
        p.ref_source = W.dev_ptr_or_null(o_so);
        p.ref_sink = W.dev_ptr_or_null(o_si);
        p.edge_chain = W.dev_ptr_or_null(o_ec);
        p.edge_state = W.dev_ptr_or_null(o_es);
        p.vertex_state = W.dev_ptr_or_null(o_vs);

        if (!stage_round_trip(h, W, L, S, "pruning", [&] { return hip_ok(h, launch_prune(p, S), "pruning kernel"); })) return PHMM_ERR_HIP;
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_prune", PHMM_FAIL_CODE)
}
