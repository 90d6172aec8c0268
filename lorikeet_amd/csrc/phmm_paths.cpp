// phmm_assembly_best_paths (include/phmm.h): host side -- validation, what the host can decide about a graph before the device
// sees it (skipped, no ends, a weight beyond the table), the node pools, the log10 table, staging, the launches and the
// hand-over if the caller's arrays hold the paths.  The cycle removal, the search, the bases and the duplicate marks run on the
// device (phmm_paths_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "phmm_paths_internal.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace phmm {

uint64_t paths_pool_size(uint32_t budget, uint64_t sources, uint32_t max_paths, uint64_t edges) {
    if (max_paths == 0xffffffffu) return edges ? budget : std::min<uint64_t>(budget, sources);
    // (max_paths - 1) * edges stays below 2^64: both factors are below 2^32; the sum can wrap only above the budget
    const uint64_t grown = (uint64_t)(max_paths - 1) * edges;
    if (grown >= budget) return budget;
    return std::min<uint64_t>(budget, sources + grown);
}

bool paths_grow_log10(std::vector<double> &table, uint64_t need) {
    if (need > PATHS_MAX_WEIGHT) return false;
    if (table.size() > need) return true;
    uint64_t size = 1024;
    while (size < need + 1) size <<= 1;
    size = std::min<uint64_t>(size, (uint64_t)PATHS_MAX_WEIGHT + 1);
    table.reserve(size);
    for (uint64_t n = table.size(); n < size; ++n) table.push_back(n ? std::log10((double)n) : -std::numeric_limits<double>::infinity());
    return true;
}

}  // namespace phmm

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_best_paths: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int phmm_assembly_best_paths(
    phmm_handle *h, uint32_t n_graphs, const uint32_t *seq_vertex_off, const uint32_t *seq_edge_off, const uint32_t *seq_base_off,
    const uint32_t *seq_vertex_base_off, const uint32_t *seq_edge_src, const uint32_t *seq_edge_dst, const uint8_t *seq_edge_is_ref,
    const uint32_t *seq_edge_multiplicity, const uint8_t *seq_bases, const uint32_t *seq_status, const uint32_t *graph_source,
    const uint32_t *graph_sink, const uint8_t *vertex_role, uint32_t max_paths, uint32_t max_nodes_per_graph, uint32_t n_regions, uint32_t n_k,
    const uint32_t *region_ref_off, const uint8_t *ref_bases, const uint32_t *capacity, uint32_t *required, uint32_t *paths_status,
    uint32_t *n_paths, uint32_t *n_popped, uint32_t *n_cycle_edges_removed, uint32_t *n_cycle_vertices_removed, uint32_t *path_off,
    uint32_t *path_edge_off, uint32_t *hap_base_off, double *path_score, uint8_t *path_is_ref, uint32_t *path_n_edges, uint32_t *hap_off,
    uint32_t *path_first_equal, uint32_t *path_edges, uint8_t *hap_bases, uint8_t *edge_removed, uint8_t *vertex_removed) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!capacity || !required) return fail(h, "a required pointer is NULL (capacity, required)");
        if (!max_paths) return fail(h, "max_paths is 0");
        if (!max_nodes_per_graph) return fail(h, "max_nodes_per_graph is 0");
        if (n_graphs > 0x7fffffffu) return fail(h, "n_graphs does not fit 31 bits");
        const bool regions = region_ref_off != nullptr;
        if (!regions && (ref_bases || n_regions || n_k)) return fail(h, "n_regions, n_k, region_ref_off and ref_bases are given together or not at all");
        if (regions && (uint64_t)n_k * n_regions != n_graphs)
            return fail(h, "n_k x n_regions = " + std::to_string((uint64_t)n_k * n_regions) + " is not n_graphs (" + std::to_string(n_graphs) + ")");
        if (path_first_equal && !regions) return fail(h, "path_first_equal is given without the region arrays");
        if (regions) {
            if (region_ref_off[0]) return fail(h, "region_ref_off does not start at 0");
            for (uint32_t r = 0; r < n_regions; ++r)
                if (region_ref_off[r + 1] < region_ref_off[r]) return fail(h, "region " + std::to_string(r) + ": region_ref_off decreases");
            if (region_ref_off[n_regions] && !ref_bases) return fail(h, "a required pointer is NULL (ref_bases)");
        }
        if (!n_graphs) {
            required[0] = required[1] = required[2] = 0;
            if (path_off) path_off[0] = 0;
            if (path_edge_off) path_edge_off[0] = 0;
            if (hap_base_off) hap_base_off[0] = 0;
            if (hap_off) hap_off[0] = 0;
            return PHMM_OK;
        }
        if (!seq_vertex_off || !seq_edge_off || !seq_base_off) return fail(h, "a required pointer is NULL (seq_vertex_off, seq_edge_off, seq_base_off)");
        if (!vertex_role && (!graph_source || !graph_sink)) return fail(h, "a required pointer is NULL (graph_source, graph_sink, or vertex_role in their place)");
        if (!paths_status || !n_paths || !n_popped || !n_cycle_edges_removed || !n_cycle_vertices_removed || !path_off || !path_edge_off || !hap_base_off)
            return fail(h, "a required pointer is NULL (the per-graph outputs)");
        if (seq_vertex_off[0]) return fail(h, "seq_vertex_off does not start at 0");
        if (seq_edge_off[0]) return fail(h, "seq_edge_off does not start at 0");
        if (seq_base_off[0]) return fail(h, "seq_base_off does not start at 0");
        for (uint32_t g = 0; g < n_graphs; ++g) {
            if (seq_vertex_off[g + 1] < seq_vertex_off[g]) return fail(h, "graph " + std::to_string(g) + ": seq_vertex_off decreases");
            if (seq_edge_off[g + 1] < seq_edge_off[g]) return fail(h, "graph " + std::to_string(g) + ": seq_edge_off decreases");
            if (seq_base_off[g + 1] < seq_base_off[g]) return fail(h, "graph " + std::to_string(g) + ": seq_base_off decreases");
        }
        const uint32_t V = seq_vertex_off[n_graphs], E = seq_edge_off[n_graphs], B = seq_base_off[n_graphs];
        if (V && !seq_vertex_base_off) return fail(h, "a required pointer is NULL (seq_vertex_base_off)");
        if (E && (!seq_edge_src || !seq_edge_dst || !seq_edge_is_ref || !seq_edge_multiplicity))
            return fail(h, "a required pointer is NULL (seq_edge_src, seq_edge_dst, seq_edge_is_ref, seq_edge_multiplicity)");
        if (B && !seq_bases) return fail(h, "a required pointer is NULL (seq_bases)");
        if ((capacity[0] && (!path_score || !path_is_ref || !path_n_edges || !hap_off)) || (capacity[1] && !path_edges) || (capacity[2] && !hap_bases))
            return fail(h, "a capacity above 0 whose arrays are NULL");
        // ... and, graph by graph, what the device need not look at, the largest total and the node pools
        std::vector<uint32_t> pre(n_graphs, PATHS_OK);
        std::vector<uint64_t> node_off((size_t)n_graphs + 1, 0), total;
        uint64_t need = 1;
        for (uint32_t g = 0; g < n_graphs; ++g) {
            const uint32_t v0 = seq_vertex_off[g], nv = seq_vertex_off[g + 1] - v0, e0 = seq_edge_off[g], ne = seq_edge_off[g + 1] - e0;
            const uint32_t nb = seq_base_off[g + 1] - seq_base_off[g];
            const auto gr = [&] { return "graph " + std::to_string(g) + ": "; };
            uint64_t sources = 0;
            for (uint32_t v = 0; v < nv; ++v) {
                const uint32_t at = seq_vertex_base_off[v0 + v];
                if (at > nb) return fail(h, gr() + "vertex " + std::to_string(v) + ": seq_vertex_base_off " + std::to_string(at) + " is past the graph's bytes (" + std::to_string(nb) + ")");
                if (v && at < seq_vertex_base_off[v0 + v - 1]) return fail(h, gr() + "vertex " + std::to_string(v) + ": seq_vertex_base_off decreases");
                if (vertex_role) {
                    if (vertex_role[v0 + v] > 3) return fail(h, gr() + "vertex " + std::to_string(v) + ": its role " + std::to_string(vertex_role[v0 + v]) + " is above 3");
                    sources += vertex_role[v0 + v] & 1;
                }
            }
            total.assign(nv, 0);
            for (uint32_t e = 0; e < ne; ++e) {
                const auto ed = [&] { return gr() + "edge " + std::to_string(e) + ": "; };
                if (seq_edge_src[e0 + e] >= nv) return fail(h, ed() + "its source " + std::to_string(seq_edge_src[e0 + e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (seq_edge_dst[e0 + e] >= nv) return fail(h, ed() + "its target " + std::to_string(seq_edge_dst[e0 + e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                total[seq_edge_src[e0 + e]] += seq_edge_multiplicity[e0 + e];
            }
            if (!vertex_role) {
                const uint32_t s = graph_source[g], t = graph_sink[g];
                if (s != PATHS_NONE && s >= nv) return fail(h, gr() + "its source " + std::to_string(s) + " is neither a vertex nor UINT32_MAX");
                if (t != PATHS_NONE && t >= nv) return fail(h, gr() + "its sink " + std::to_string(t) + " is neither a vertex nor UINT32_MAX");
                sources = 1;
                if (s == PATHS_NONE || t == PATHS_NONE) pre[g] = PATHS_NO_ENDS;
            }
            if (seq_status && seq_status[g] != PHMM_SEQ_OK) pre[g] = PATHS_SKIPPED;
            const uint64_t largest = nv ? *std::max_element(total.begin(), total.end()) : 0;
            if (pre[g] == PATHS_OK && largest > PATHS_MAX_WEIGHT) pre[g] = PATHS_WEIGHT_RANGE;
            if (pre[g] == PATHS_OK) need = std::max(need, largest);
            node_off[g + 1] = node_off[g] + (pre[g] == PATHS_OK ? paths_pool_size(max_nodes_per_graph, sources, max_paths, ne) : 0);
        }
        const uint64_t nodes = node_off[n_graphs];
        if (nodes > 0xffffffffull) return fail(h, "the node pools of the call do not fit 32 bits (" + std::to_string(nodes) + " nodes): lower max_nodes_per_graph or split the call");
        const uint32_t n_ref = regions ? region_ref_off[n_regions] : 0;
        if (!paths_grow_log10(h->paths_log10, need)) throw std::logic_error("a total above the table's range was let through");

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->paths_staging;
        hipStream_t S = h->streams[0];
        // ---- the table, grown to the largest total this handle has met ---------------------------------------------------------
        StageLayout T;
        const auto t_log = T.scratch<double>(h->paths_log10.size());
        if (h->paths_log10_on_device < h->paths_log10.size()) {
            if (!h->paths_table.reserve(h, T, "log10 table")) return PHMM_ERR_HIP;
            if (!hip_ok(h, hipMemcpy(h->paths_table.ptr(t_log), h->paths_log10.data(), 8 * h->paths_log10.size(), hipMemcpyHostToDevice), "H2D log10 table"))
                return PHMM_ERR_HIP;
            h->paths_log10_on_device = h->paths_log10.size();
        }
        // ---- staging: inputs, then the results; the trees, queues and marks lie in the device-only workspace -------------------
        StageLayout L;
        const auto s_vo = L.in(seq_vertex_off, (size_t)n_graphs + 1), s_eo = L.in(seq_edge_off, (size_t)n_graphs + 1), s_bo = L.in(seq_base_off, (size_t)n_graphs + 1);
        const auto s_no = L.in(node_off.data(), (size_t)n_graphs + 1);
        const auto s_pre = L.in(pre.data(), n_graphs);
        const auto s_src = L.in(graph_source, vertex_role ? 0 : n_graphs), s_snk = L.in(graph_sink, vertex_role ? 0 : n_graphs);
        const auto s_vb = L.in(seq_vertex_base_off, V);
        const auto s_es = L.in(seq_edge_src, E), s_ed = L.in(seq_edge_dst, E), s_em = L.in(seq_edge_multiplicity, E);
        const auto s_er = L.in(seq_edge_is_ref, E);
        const auto s_role = L.in(vertex_role, vertex_role ? V : 0);
        const auto s_sb = L.in(seq_bases, B);
        const auto s_ro = L.in(region_ref_off, regions ? (size_t)n_regions + 1 : 0);
        const auto s_rb = L.in(ref_bases, n_ref);
        L.end_inputs();
        const auto o_counts = L.out<uint32_t>((size_t)PATHS_COUNTS * n_graphs), o_off = L.out<uint32_t>(3 * ((size_t)n_graphs + 1)), o_fits = L.out<uint32_t>(1);
        const auto o_sc = L.out<double>(capacity[0]);
        const auto o_ne = L.out<uint32_t>(capacity[0]), o_ho = L.out<uint32_t>((size_t)capacity[0] + 1);
        const auto o_fe = L.out<uint32_t>(path_first_equal ? capacity[0] : 0);
        const auto o_ir = L.out<uint8_t>(capacity[0]);
        const auto o_pe = L.out<uint32_t>(capacity[1]);
        const auto o_hb = L.out<uint8_t>(capacity[2]);
        StageLayout D;  // the device-only workspace: 20 bytes per vertex, 4 per edge, 45 per node
        const auto o_egone = out_or_scratch(L, D, edge_removed, E, true), o_vgone = out_or_scratch(L, D, vertex_removed, V, true);
        const auto w_v = D.scratch<uint32_t>((size_t)PATHS_VERTEX_WORDS * ((size_t)V + n_graphs));
        const auto w_csr = D.scratch<uint32_t>(E);
        const auto w_reach = D.scratch<uint8_t>(V);
        const auto w_np = D.scratch<uint32_t>(nodes), w_ne = D.scratch<uint32_t>(nodes), w_nv = D.scratch<uint32_t>(nodes), w_nl = D.scratch<uint32_t>(nodes);
        const auto w_nb = D.scratch<uint32_t>(nodes), w_qn = D.scratch<uint32_t>(nodes), w_rn = D.scratch<uint32_t>(nodes);
        const auto w_ns = D.scratch<double>(nodes);
        const auto w_qk = D.scratch<uint64_t>(nodes);
        const auto w_nr = D.scratch<uint8_t>(nodes);
        if (!h->paths_scratch.reserve(h, D, "best paths workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "best paths staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->paths_scratch;

        PathsParams p{};
        p.n_graphs = n_graphs;
        p.n_regions = regions ? n_regions : 0;
        p.vertex_off = W.dev_ptr(s_vo);
        p.edge_off = W.dev_ptr(s_eo);
        p.base_off = W.dev_ptr(s_bo);
        p.vertex_base_off = W.dev_ptr(s_vb);
        p.edge_src = W.dev_ptr(s_es);
        p.edge_dst = W.dev_ptr(s_ed);
        p.edge_mult = W.dev_ptr(s_em);
        p.edge_is_ref = W.dev_ptr(s_er);
        p.bases = W.dev_ptr(s_sb);
        p.pre_status = W.dev_ptr(s_pre);
        p.graph_source = vertex_role ? nullptr : W.dev_ptr(s_src);
        p.graph_sink = vertex_role ? nullptr : W.dev_ptr(s_snk);
        p.vertex_role = vertex_role ? W.dev_ptr(s_role) : nullptr;
        p.max_paths = max_paths;
        p.max_nodes = max_nodes_per_graph;
        p.node_off = W.dev_ptr(s_no);
        p.log10_table = h->paths_table.ptr(t_log);
        p.region_ref_off = regions ? W.dev_ptr(s_ro) : nullptr;
        p.ref_bases = W.dev_ptr(s_rb);
        for (int i = 0; i < 3; ++i) p.capacity[i] = capacity[i];
        p.w = ws.ptr(w_v);
        p.w_stride = (uint64_t)V + n_graphs;
        p.e_csr = ws.ptr(w_csr);
        p.stack_reach = ws.ptr(w_reach);
        p.n_parent = ws.ptr(w_np);
        p.n_edge = ws.ptr(w_ne);
        p.n_vertex = ws.ptr(w_nv);
        p.n_len = ws.ptr(w_nl);
        p.n_bytes = ws.ptr(w_nb);
        p.n_score = ws.ptr(w_ns);
        p.n_is_ref = ws.ptr(w_nr);
        p.q_key = ws.ptr(w_qk);
        p.q_node = ws.ptr(w_qn);
        p.r_node = ws.ptr(w_rn);
        p.edge_removed = o_egone.dev_ptr(W, ws);
        p.vertex_removed = o_vgone.dev_ptr(W, ws);
        p.g_counts = W.dev_ptr(o_counts);
        p.out_off = W.dev_ptr(o_off);
        p.fits = W.dev_ptr(o_fits);
        p.path_score = W.dev_ptr(o_sc);
        p.path_is_ref = W.dev_ptr(o_ir);
        p.path_n_edges = W.dev_ptr(o_ne);
        p.path_first_equal = path_first_equal ? W.dev_ptr(o_fe) : nullptr;
        p.hap_off = W.dev_ptr(o_ho);
        p.path_edges = W.dev_ptr(o_pe);
        p.hap_bases = W.dev_ptr(o_hb);

        if (!stage_round_trip(h, W, L, S, "best paths", [&] { return hip_ok(h, launch_paths(p, S), "best paths kernels"); })) return PHMM_ERR_HIP;

        // ---- the sizes; then, if everything fits, the paths -------------------------------------------------------------------
        const uint32_t *counts = W.host_ptr(o_counts), *off = W.host_ptr(o_off);
        if (*W.host_ptr(o_fits) == PATHS_FITS_OVERFLOW)  // no capacity could hold them: not PHMM_ERR_EVENT_CAPACITY, and nothing is written
            return fail(h, "the paths, path edges or haplotype bytes of the call do not fit 32 bits: lower max_paths or split the call");
        for (int i = 0; i < 3; ++i) required[i] = off[(size_t)i * (n_graphs + 1) + n_graphs];
        if (*W.host_ptr(o_fits) != PATHS_FITS_YES) {
            h->err = "phmm_assembly_best_paths: an output array is too small (required holds the sizes)";
            return h->err_code = PHMM_ERR_EVENT_CAPACITY;
        }
        uint32_t *const per_graph[5] = {paths_status, n_paths, n_popped, n_cycle_edges_removed, n_cycle_vertices_removed};
        for (uint32_t g = 0; g < n_graphs; ++g)
            for (int i = 0; i < 5; ++i) per_graph[i][g] = counts[(size_t)PATHS_COUNTS * g + i];
        memcpy(path_off, off, 4 * ((size_t)n_graphs + 1));
        memcpy(path_edge_off, off + n_graphs + 1, 4 * ((size_t)n_graphs + 1));
        memcpy(hap_base_off, off + 2 * ((size_t)n_graphs + 1), 4 * ((size_t)n_graphs + 1));
        if (hap_off) memcpy(hap_off, W.host_ptr(o_ho), 4 * ((size_t)required[0] + 1));
        if (required[0]) {
            memcpy(path_score, W.host_ptr(o_sc), 8ull * required[0]);
            memcpy(path_is_ref, W.host_ptr(o_ir), required[0]);
            memcpy(path_n_edges, W.host_ptr(o_ne), 4ull * required[0]);
            if (path_first_equal) memcpy(path_first_equal, W.host_ptr(o_fe), 4ull * required[0]);
        }
        if (required[1]) memcpy(path_edges, W.host_ptr(o_pe), 4ull * required[1]);
        if (required[2]) memcpy(hap_bases, W.host_ptr(o_hb), required[2]);
        if (edge_removed && E) memcpy(edge_removed, W.host_ptr(o_egone.slot), E);
        if (vertex_removed && V) memcpy(vertex_removed, W.host_ptr(o_vgone.slot), V);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_best_paths", PHMM_FAIL_CODE)
}
