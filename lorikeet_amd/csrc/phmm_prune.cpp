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

struct Out {  // an output array: where it lies in the staging buffer
    void *user;
    size_t bytes;
    size_t off = 0;
};

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
        Out outs[10] = {{graph_flags, 4ull * n_graphs},     {n_chains, 4ull * n_graphs},     {n_chains_removed, 4ull * n_graphs},
                        {n_vertices_left, 4ull * n_graphs}, {n_edges_left, 4ull * n_graphs}, {ref_source, 4ull * n_graphs},
                        {ref_sink, 4ull * n_graphs},        {edge_chain, 4ull * E},          {edge_state, E},
                        {vertex_state, V}};
        for (Out &o : outs) o.off = L.out<char>(o.bytes).off;
        StageLayout D;  // the device-only workspace: 20 bytes per vertex, 5 per edge
        const auto w_vi = D.scratch<uint32_t>(V), w_vu = D.scratch<uint32_t>(V), w_ve = D.scratch<uint32_t>(V), w_vr = D.scratch<uint32_t>(V), w_vm = D.scratch<uint32_t>(V);
        const auto w_ep = D.scratch<uint32_t>(E);
        const auto w_eb = D.scratch<uint8_t>(E);
        if (h->prune_scratch_cap < D.total) {
            for (int i = 0; i < kSlots; ++i) (void)hipStreamSynchronize(h->streams[i]);
            if (h->prune_scratch) (void)hipFree(h->prune_scratch);
            h->prune_scratch = nullptr;
            h->prune_scratch_cap = 0;
            const size_t bytes = D.total + D.total / 2;
            char *ws = nullptr;
            if (!hip_ok(h, hipMalloc((void **)&ws, bytes), "hipMalloc(pruning workspace)")) return PHMM_ERR_HIP;
            h->prune_scratch = ws;
            h->prune_scratch_cap = bytes;
        }
        if (!W.reserve(h, L, "pruning staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        char *const ws = h->prune_scratch;
        auto out_ptr = [&](int i) -> void * { return outs[i].bytes ? W.dev + outs[i].off : nullptr; };

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
        p.v_in = (uint32_t *)(ws + w_vi.off);
        p.v_out = (uint32_t *)(ws + w_vu.off);
        p.v_inedge = (uint32_t *)(ws + w_ve.off);
        p.v_ref = (uint32_t *)(ws + w_vr.off);
        p.v_mark = (uint32_t *)(ws + w_vm.off);
        p.e_ptr = (uint32_t *)(ws + w_ep.off);
        p.e_bits = (uint8_t *)(ws + w_eb.off);
        p.graph_flags = (uint32_t *)out_ptr(0);
        p.n_chains = (uint32_t *)out_ptr(1);
        p.n_chains_removed = (uint32_t *)out_ptr(2);
        p.n_vertices_left = (uint32_t *)out_ptr(3);
        p.n_edges_left = (uint32_t *)out_ptr(4);
        p.ref_source = (uint32_t *)out_ptr(5);
        p.ref_sink = (uint32_t *)out_ptr(6);
        p.edge_chain = (uint32_t *)out_ptr(7);
        p.edge_state = (uint8_t *)out_ptr(8);
        p.vertex_state = (uint8_t *)out_ptr(9);

        if (!hip_ok(h, hipMemcpyAsync(W.dev, W.host, L.in_bytes, hipMemcpyHostToDevice, S), "H2D pruning") ||
            !hip_ok(h, launch_prune(p, S), "pruning kernel") ||
            !hip_ok(h, hipMemcpyAsync(W.host + L.out_begin, W.dev + L.out_begin, L.total - L.out_begin, hipMemcpyDeviceToHost, S), "D2H pruning") ||
            !hip_ok(h, hipStreamSynchronize(S), "sync(pruning)"))
            return PHMM_ERR_HIP;
        for (const Out &o : outs)
            if (o.bytes) memcpy(o.user, W.host + o.off, o.bytes);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_prune", PHMM_FAIL_CODE)
}
