// phmm_assembly_seqgraph (include/phmm.h): host side -- validation, where every vertex's bytes lie, staging, the launches, and
// the hand-over of the zipped graphs if the caller's arrays hold them.  Every step of the conversion, the clean-up and the zip
// runs on the device (phmm_seqgraph_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "phmm_seqgraph_internal.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_seqgraph: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

uint64_t pow2_ceil(uint64_t n) {
    uint64_t p = 1;
    while (p < n) p <<= 1;
    return n ? p : 0;
}

}  // namespace

extern "C" int phmm_assembly_seqgraph(
    phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases, const uint32_t *region_read_off,
    const uint32_t *read_off, const uint8_t *read_bases, const uint32_t *read_first, const uint32_t *read_len, uint32_t n_k,
    const uint32_t *k, const uint32_t *vertex_off, const uint32_t *edge_off, const uint32_t *vertex_seq, const uint32_t *vertex_pos,
    const uint32_t *edge_src, const uint32_t *edge_dst, const uint8_t *edge_is_ref, const uint32_t *edge_multiplicity,
    const uint32_t *new_vertex_off, const uint8_t *new_vertex_kmer, const uint8_t *vertex_absent, const uint8_t *edge_absent,
    const uint32_t *graph_flags, const uint32_t *capacity, uint32_t *required, uint32_t *seq_status, uint32_t *n_seq_vertices,
    uint32_t *n_seq_edges, uint32_t *n_seq_bases, uint32_t *n_chains_zipped, uint32_t *n_removed_clean, uint32_t *n_removed_unconnected,
    uint32_t *seq_ref_source, uint32_t *seq_ref_sink, uint32_t *seq_vertex_off, uint32_t *seq_edge_off, uint32_t *seq_base_off,
    uint32_t *seq_vertex_base_off, uint32_t *seq_vertex_first, uint32_t *seq_vertex_n_merged, uint32_t *seq_edge_src, uint32_t *seq_edge_dst,
    uint8_t *seq_edge_is_ref, uint32_t *seq_edge_multiplicity, uint8_t *seq_bases, uint32_t *vertex_to_seq) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!capacity || !required) return fail(h, "a required pointer is NULL (capacity, required)");
        if (!vertex_absent != !edge_absent) return fail(h, "vertex_absent and edge_absent are given together or not at all");
        if (!new_vertex_off != !new_vertex_kmer) return fail(h, "new_vertex_off and new_vertex_kmer are given together or not at all");
        if ((uint64_t)n_k * n_regions > 0x7fffffffull) return fail(h, "n_k x n_regions does not fit 31 bits");
        const uint32_t n_graphs = n_k * n_regions;
        if (!n_graphs) {
            required[0] = required[1] = required[2] = 0;
            if (seq_vertex_off) seq_vertex_off[0] = 0;
            if (seq_edge_off) seq_edge_off[0] = 0;
            if (seq_base_off) seq_base_off[0] = 0;
            return PHMM_OK;
        }
        if (!k) return fail(h, "a required pointer is NULL (k)");
        uint32_t k_max = 0;
        for (uint32_t i = 0; i < n_k; ++i) {
            if (k[i] < 1 || k[i] > PHMM_ASM_MAX_K) return fail(h, "k[" + std::to_string(i) + "] = " + std::to_string(k[i]) + " is outside 1 .. " + std::to_string(PHMM_ASM_MAX_K));
            k_max = std::max(k_max, k[i]);
        }
        if (!region_ref_off || !region_read_off) return fail(h, "a required pointer is NULL (region_ref_off, region_read_off)");
        if (region_ref_off[0]) return fail(h, "region_ref_off does not start at 0");
        if (region_read_off[0]) return fail(h, "region_read_off does not start at 0");
        for (uint32_t r = 0; r < n_regions; ++r) {
            if (region_ref_off[r + 1] < region_ref_off[r]) return fail(h, "region " + std::to_string(r) + ": region_ref_off decreases");
            if (region_read_off[r + 1] < region_read_off[r]) return fail(h, "region " + std::to_string(r) + ": region_read_off decreases");
        }
        const uint32_t n_ref = region_ref_off[n_regions], n_reads = region_read_off[n_regions];
        if (n_ref && !ref_bases) return fail(h, "a required pointer is NULL (ref_bases)");
        if (n_reads && !read_off) return fail(h, "a required pointer is NULL (read_off)");
        if (!read_first != !read_len) return fail(h, "read_first and read_len are given together or not at all");
        if (n_reads && read_off[0]) return fail(h, "read_off does not start at 0");
        for (uint32_t r = 0; r < n_reads; ++r) {
            if (read_off[r + 1] < read_off[r]) return fail(h, "read " + std::to_string(r) + ": read_off decreases");
            if (read_first && (uint64_t)read_first[r] + read_len[r] > read_off[r + 1] - read_off[r])
                return fail(h, "read " + std::to_string(r) + ": its window leaves the read");
        }
        const uint32_t n_read_bases = n_reads ? read_off[n_reads] : 0;
        if (n_read_bases && !read_bases) return fail(h, "a required pointer is NULL (read_bases)");
        if (!vertex_off || !edge_off) return fail(h, "a required pointer is NULL (vertex_off, edge_off)");
        if (!seq_status || !n_seq_vertices || !n_seq_edges || !n_seq_bases || !n_chains_zipped || !n_removed_clean || !n_removed_unconnected ||
            !seq_ref_source || !seq_ref_sink || !seq_vertex_off || !seq_edge_off || !seq_base_off)
            return fail(h, "a required pointer is NULL (the per-graph outputs)");
        if (vertex_off[0]) return fail(h, "vertex_off does not start at 0");
        if (edge_off[0]) return fail(h, "edge_off does not start at 0");
        if (new_vertex_off && new_vertex_off[0]) return fail(h, "new_vertex_off does not start at 0");
        for (uint32_t g = 0; g < n_graphs; ++g) {
            if (vertex_off[g + 1] < vertex_off[g]) return fail(h, "graph " + std::to_string(g) + ": vertex_off decreases");
            if (edge_off[g + 1] < edge_off[g]) return fail(h, "graph " + std::to_string(g) + ": edge_off decreases");
            if (vertex_off[g + 1] - vertex_off[g] >= SEQ_MAX_VERTICES) return fail(h, "graph " + std::to_string(g) + ": its vertices do not fit 31 bits");
            if (new_vertex_off) {
                if (new_vertex_off[g + 1] < new_vertex_off[g]) return fail(h, "graph " + std::to_string(g) + ": new_vertex_off decreases");
                if (new_vertex_off[g + 1] - new_vertex_off[g] > vertex_off[g + 1] - vertex_off[g])
                    return fail(h, "graph " + std::to_string(g) + ": more new vertices than vertices");
            }
        }
        const uint32_t V = vertex_off[n_graphs], E = edge_off[n_graphs], NV = new_vertex_off ? new_vertex_off[n_graphs] : 0;
        if (V - NV && (!vertex_seq || !vertex_pos)) return fail(h, "a required pointer is NULL (vertex_seq, vertex_pos)");
        if (E && (!edge_src || !edge_dst || !edge_is_ref || !edge_multiplicity))
            return fail(h, "a required pointer is NULL (edge_src, edge_dst, edge_is_ref, edge_multiplicity)");
        if ((uint64_t)V * k_max > 0xffffffffull) return fail(h, "vertices x max k does not fit 32 bits: the sequence bytes could not be counted");
        const uint64_t kmer_bytes = (uint64_t)NV * k_max;
        // (the vertex bases index one array: behind the reference's slot the reads' slot, then the rows' slot, each at a multiple of 256)
        const uint64_t reads_at = up256(n_ref), rows_at = reads_at + up256(n_read_bases);
        if (rows_at + kmer_bytes > 0xffffffffull) return fail(h, "the bases do not fit 32 bits");
        std::vector<uint32_t> vertex_base(V, 0), key_off(n_graphs + 1, 0);
        for (uint32_t g = 0; g < n_graphs; ++g) {
            const uint32_t v0 = vertex_off[g], nv = vertex_off[g + 1] - v0, reg = g % n_regions, kk = k[g / n_regions];
            const uint32_t reads0 = region_read_off[reg], nr = region_read_off[reg + 1] - reads0;
            const uint32_t n_new = new_vertex_off ? new_vertex_off[g + 1] - new_vertex_off[g] : 0, n_raw = nv - n_new;
            const uint32_t raw0 = v0 - (new_vertex_off ? new_vertex_off[g] : 0);  // where the graph's rows of vertex_seq / vertex_pos start
            for (uint32_t v = 0; v < nv; ++v) {
                if (vertex_absent && vertex_absent[v0 + v]) continue;
                if (v >= n_raw) {  // a vertex recovery made: its bytes are its row's
                    vertex_base[v0 + v] = (uint32_t)(rows_at + (uint64_t)(new_vertex_off[g] + (v - n_raw)) * k_max);
                    continue;
                }
                const auto vx = [&] { return "graph " + std::to_string(g) + ": vertex " + std::to_string(v) + ": "; };
                const uint32_t sq = vertex_seq[raw0 + v], pos = vertex_pos[raw0 + v];
                if (sq > nr) return fail(h, vx() + "its sequence " + std::to_string(sq) + " is not one of the region's (" + std::to_string(nr) + " reads)");
                uint32_t start, len;
                if (sq == 0) {
                    start = region_ref_off[reg];
                    len = region_ref_off[reg + 1] - start;
                } else {
                    const uint32_t r = reads0 + sq - 1;
                    start = (uint32_t)reads_at + read_off[r] + (read_first ? read_first[r] : 0);
                    len = read_first ? read_len[r] : read_off[r + 1] - read_off[r];
                }
                if ((uint64_t)pos + kk > len) return fail(h, vx() + "its bytes [" + std::to_string(pos) + ", +" + std::to_string(kk) + ") leave their sequence (" + std::to_string(len) + " bases)");
                vertex_base[v0 + v] = start + pos;
            }
            for (uint32_t e = edge_off[g]; e < edge_off[g + 1]; ++e) {
                const auto ed = [&] { return "graph " + std::to_string(g) + ": edge " + std::to_string(e - edge_off[g]) + ": "; };
                if (edge_src[e] >= nv) return fail(h, ed() + "its source " + std::to_string(edge_src[e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (edge_dst[e] >= nv) return fail(h, ed() + "its target " + std::to_string(edge_dst[e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (edge_absent && !edge_absent[e] && (vertex_absent[v0 + edge_src[e]] || vertex_absent[v0 + edge_dst[e]]))
                    return fail(h, ed() + "it is present and an endpoint is absent");
            }
            const uint64_t slots = key_off[g] + pow2_ceil(edge_off[g + 1] - edge_off[g]);
            if (slots > 0xffffffffull) return fail(h, "graph " + std::to_string(g) + ": the sort slots do not fit 32 bits");
            key_off[g + 1] = (uint32_t)slots;
        }
        if ((capacity[0] && (!seq_vertex_base_off || !seq_vertex_first || !seq_vertex_n_merged)) ||
            (capacity[1] && (!seq_edge_src || !seq_edge_dst || !seq_edge_is_ref || !seq_edge_multiplicity)) || (capacity[2] && !seq_bases))
            return fail(h, "a capacity above 0 whose arrays are NULL");

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->seqgraph_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the results; the graphs' state lies in the device-only workspace --------------------------------
        StageLayout L;
        const auto s_rb = L.in(ref_bases, n_ref), s_qb = L.in(read_bases, n_read_bases), s_nk = L.in(new_vertex_kmer, (size_t)kmer_bytes);
        const auto s_k = L.in(k, n_k);
        const auto s_vo = L.in(vertex_off, (size_t)n_graphs + 1), s_eo = L.in(edge_off, (size_t)n_graphs + 1), s_ko = L.in(key_off.data(), (size_t)n_graphs + 1);
        const auto s_vb = L.in(vertex_base.data(), V);
        const auto s_es = L.in(edge_src, E), s_ed = L.in(edge_dst, E), s_em = L.in(edge_multiplicity, E);
        const auto s_er = L.in(edge_is_ref, E);
        const auto s_va = L.in(vertex_absent, vertex_absent ? V : 0), s_ea = L.in(edge_absent, edge_absent ? E : 0);
        const auto s_gf = L.in(graph_flags, graph_flags ? n_graphs : 0);
        L.end_inputs();
        if (s_qb.off - s_rb.off != reads_at || s_nk.off - s_rb.off != rows_at) throw std::logic_error("the bases' slots are not where the vertex bases expect them");
        const auto o_counts = L.out<uint32_t>((size_t)SEQ_COUNTS * n_graphs), o_off = L.out<uint32_t>(3 * ((size_t)n_graphs + 1)), o_fits = L.out<uint32_t>(1);
        const auto o_vb = L.out<uint32_t>(capacity[0]), o_vf = L.out<uint32_t>(capacity[0]), o_vn = L.out<uint32_t>(capacity[0]);
        const auto o_es = L.out<uint32_t>(capacity[1]), o_ed = L.out<uint32_t>(capacity[1]), o_em = L.out<uint32_t>(capacity[1]);
        const auto o_er = L.out<uint8_t>(capacity[1]);
        const auto o_sb = L.out<uint8_t>(capacity[2]);
        StageLayout D;  // the device-only workspace: 84 bytes per vertex, 5 per edge, 16 per sort slot
        const auto o_ts = out_or_scratch(L, D, vertex_to_seq, V, true);
        const auto w_v = D.scratch<uint32_t>((size_t)SEQ_VERTEX_WORDS * V);
        const auto w_ep = D.scratch<uint32_t>(E);
        const auto w_ee = D.scratch<uint8_t>(E);
        const auto w_key = D.scratch<uint64_t>(2 * (size_t)key_off[n_graphs]);
        if (!h->seqgraph_scratch.reserve(h, D, "sequence graph workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "sequence graph staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->seqgraph_scratch;

        SeqParams p{};
        p.n_graphs = n_graphs;
        p.n_regions = n_regions;
        p.k = W.dev_ptr(s_k);
        p.vertex_off = W.dev_ptr(s_vo);
        p.edge_off = W.dev_ptr(s_eo);
        p.key_off = W.dev_ptr(s_ko);
        p.bases = W.dev_ptr(s_rb);
        p.vertex_base = W.dev_ptr(s_vb);
        p.edge_src = W.dev_ptr(s_es);
        p.edge_dst = W.dev_ptr(s_ed);
        p.edge_mult = W.dev_ptr(s_em);
        p.edge_is_ref = W.dev_ptr(s_er);
        p.vertex_absent = vertex_absent ? W.dev_ptr(s_va) : nullptr;
        p.edge_absent = edge_absent ? W.dev_ptr(s_ea) : nullptr;
        p.graph_flags = graph_flags ? W.dev_ptr(s_gf) : nullptr;
        for (int i = 0; i < 3; ++i) p.capacity[i] = capacity[i];
        p.w = ws.ptr(w_v);
        p.v_total = V;
        p.e_state = ws.ptr(w_ee);
        p.e_pos = ws.ptr(w_ep);
        p.keys = ws.ptr(w_key);
        p.g_counts = W.dev_ptr(o_counts);
        p.seq_off = W.dev_ptr(o_off);
        p.fits = W.dev_ptr(o_fits);
        p.sv_base_off = W.dev_ptr(o_vb);
        p.sv_first = W.dev_ptr(o_vf);
        p.sv_n_merged = W.dev_ptr(o_vn);
        p.se_src = W.dev_ptr(o_es);
        p.se_dst = W.dev_ptr(o_ed);
        p.se_mult = W.dev_ptr(o_em);
        p.se_is_ref = W.dev_ptr(o_er);
        p.seq_bases = W.dev_ptr(o_sb);
        p.vertex_to_seq = o_ts.dev_ptr(W, ws);

        if (!stage_round_trip(h, W, L, S, "sequence graphs", [&] { return hip_ok(h, launch_seqgraph(p, S), "sequence graph kernels"); })) return PHMM_ERR_HIP;

        // ---- the sizes; then, if everything fits, the graphs ---------------------------------------------------------------------
        const uint32_t *counts = W.host_ptr(o_counts), *off = W.host_ptr(o_off);
        for (int i = 0; i < 3; ++i) required[i] = off[(size_t)i * (n_graphs + 1) + n_graphs];
        if (!*W.host_ptr(o_fits)) {
            h->err = "phmm_assembly_seqgraph: an output array is too small (required holds the sizes)";
            return h->err_code = PHMM_ERR_EVENT_CAPACITY;
        }
        uint32_t *const per_graph[SEQ_COUNTS] = {seq_status, n_seq_vertices, n_seq_edges, n_seq_bases, n_chains_zipped, n_removed_clean, n_removed_unconnected,
                                                 seq_ref_source, seq_ref_sink};
        for (uint32_t g = 0; g < n_graphs; ++g)
            for (int i = 0; i < SEQ_COUNTS; ++i) per_graph[i][g] = counts[(size_t)SEQ_COUNTS * g + i];
        memcpy(seq_vertex_off, off, 4 * ((size_t)n_graphs + 1));
        memcpy(seq_edge_off, off + n_graphs + 1, 4 * ((size_t)n_graphs + 1));
        memcpy(seq_base_off, off + 2 * ((size_t)n_graphs + 1), 4 * ((size_t)n_graphs + 1));
        if (required[0]) {
            memcpy(seq_vertex_base_off, W.host_ptr(o_vb), 4ull * required[0]);
            memcpy(seq_vertex_first, W.host_ptr(o_vf), 4ull * required[0]);
            memcpy(seq_vertex_n_merged, W.host_ptr(o_vn), 4ull * required[0]);
        }
        if (required[1]) {
            memcpy(seq_edge_src, W.host_ptr(o_es), 4ull * required[1]);
            memcpy(seq_edge_dst, W.host_ptr(o_ed), 4ull * required[1]);
            memcpy(seq_edge_multiplicity, W.host_ptr(o_em), 4ull * required[1]);
            memcpy(seq_edge_is_ref, W.host_ptr(o_er), required[1]);
        }
        if (required[2]) memcpy(seq_bases, W.host_ptr(o_sb), required[2]);
        if (vertex_to_seq && V) memcpy(vertex_to_seq, W.host_ptr(o_ts.slot), 4ull * V);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_seqgraph", PHMM_FAIL_CODE)
}
