// phmm_assembly_recover (include/phmm.h): host side -- validation, sizing, staging, one launch, and the cut of the device's
// slots down to what the graphs gained.  Every step of the recovery runs on the device (phmm_recover_kernels.hip); there is no
// CPU path here.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "phmm_recover_internal.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_recover: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

constexpr size_t kSlabBudget = 512ull << 20;  // bytes of aligner slabs a call may hold: bounds the workgroups in flight
constexpr uint32_t kMaxBlocks = 1024;

}  // namespace

extern "C" int phmm_assembly_recover(
    phmm_handle *h, const void *cfg_v, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
    const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases, const uint32_t *read_first,
    const uint32_t *read_len, uint32_t n_k, const uint32_t *k, const uint32_t *vertex_off, const uint32_t *edge_off,
    const uint32_t *vertex_seq, const uint32_t *vertex_pos, const uint32_t *edge_src, const uint32_t *edge_dst,
    const uint8_t *edge_is_ref, const uint32_t *edge_multiplicity, const uint32_t *edge_pruning_multiplicity,
    const uint8_t *vertex_absent, const uint8_t *edge_absent, const uint32_t *graph_flags, const uint32_t *prune_factor,
    const uint32_t *capacity, uint32_t *required, uint32_t *n_tails, uint32_t *n_tails_recovered, uint32_t *n_heads,
    uint32_t *n_heads_recovered, uint32_t *n_new_edges, uint32_t *n_new_vertices, uint32_t *n_rounds, uint32_t *end_off,
    uint32_t *new_edge_off, uint32_t *new_vertex_off, uint32_t *end_vertex, uint32_t *end_kind, uint32_t *end_status,
    uint32_t *end_alt_len, uint32_t *end_ref_len, uint32_t *end_n_cigar, uint32_t *end_cigar, uint32_t *end_edge,
    uint32_t *new_edge_src, uint32_t *new_edge_dst, uint32_t *new_edge_multiplicity, uint32_t *new_edge_pruning_multiplicity,
    uint8_t *new_vertex_kmer, uint8_t *edge_removed) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!cfg_v) return fail(h, "a required pointer is NULL (cfg)");
        const phmm_recover_config cfg = *static_cast<const phmm_recover_config *>(cfg_v);
        if (!cfg.ops) return fail(h, "ops is 0: nothing is asked for");
        if (cfg.ops & ~(PHMM_RECOVER_OP_TAILS | PHMM_RECOVER_OP_HEADS)) return fail(h, "ops has unknown bits (" + std::to_string(cfg.ops) + ")");
        if (cfg.num_pruning_samples < 1 || cfg.num_pruning_samples > PHMM_GRAPH_MAX_PRUNING_SAMPLES)
            return fail(h, "num_pruning_samples (" + std::to_string(cfg.num_pruning_samples) + ") is outside 1 .. " + std::to_string(PHMM_GRAPH_MAX_PRUNING_SAMPLES));
        if (!capacity || !required) return fail(h, "a required pointer is NULL (capacity, required)");
        if (!vertex_absent != !edge_absent) return fail(h, "vertex_absent and edge_absent are given together or not at all");
        if ((uint64_t)n_k * n_regions > 0x7fffffffull) return fail(h, "n_k x n_regions does not fit 31 bits");
        const uint32_t n_graphs = n_k * n_regions;
        if (!n_graphs) {
            required[0] = required[1] = required[2] = 0;
            if (end_off) end_off[0] = 0;
            if (new_edge_off) new_edge_off[0] = 0;
            if (new_vertex_off) new_vertex_off[0] = 0;
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
        if ((uint64_t)n_ref + n_read_bases > 0xffffffffull) return fail(h, "the bases do not fit 32 bits");
        if (!vertex_off || !edge_off) return fail(h, "a required pointer is NULL (vertex_off, edge_off)");
        if (!prune_factor) return fail(h, "a required pointer is NULL (prune_factor)");
        if (!n_tails || !n_tails_recovered || !n_heads || !n_heads_recovered || !n_new_edges || !n_new_vertices || !n_rounds || !end_off ||
            !new_edge_off || !new_vertex_off)
            return fail(h, "a required pointer is NULL (the per-graph outputs)");
        if (vertex_off[0]) return fail(h, "vertex_off does not start at 0");
        if (edge_off[0]) return fail(h, "edge_off does not start at 0");
        for (uint32_t g = 0; g < n_graphs; ++g) {
            if (vertex_off[g + 1] < vertex_off[g]) return fail(h, "graph " + std::to_string(g) + ": vertex_off decreases");
            if (edge_off[g + 1] < edge_off[g]) return fail(h, "graph " + std::to_string(g) + ": edge_off decreases");
            if (vertex_off[g + 1] - vertex_off[g] > RECOVER_MAX_VERTICES)
                return fail(h, "graph " + std::to_string(g) + ": more than " + std::to_string(RECOVER_MAX_VERTICES) + " vertices");
            if (graph_flags && (graph_flags[g] & PHMM_PRUNE_HAS_CYCLE)) return fail(h, "graph " + std::to_string(g) + ": it is flagged cyclic (PHMM_PRUNE_HAS_CYCLE)");
        }
        const uint32_t V = vertex_off[n_graphs], E = edge_off[n_graphs];
        if (V && (!vertex_seq || !vertex_pos)) return fail(h, "a required pointer is NULL (vertex_seq, vertex_pos)");
        if (E && (!edge_src || !edge_dst || !edge_is_ref || !edge_multiplicity || !edge_pruning_multiplicity))
            return fail(h, "a required pointer is NULL (edge_src, edge_dst, edge_is_ref, edge_multiplicity, edge_pruning_multiplicity)");
        if (E && !edge_removed) return fail(h, "a required pointer is NULL (edge_removed)");
        // degrees of the graphs as given: what bounds the ends, and with them the edges and vertices the call can make
        std::vector<uint32_t> deg_in(V, 0), deg_out(V, 0), vertex_base(V, 0);
        std::vector<uint8_t> ref_bits(V, 0);
        std::vector<uint32_t> xv_off(n_graphs + 1, 0), xe_off(n_graphs + 1, 0), xend_off(n_graphs + 1, 0);
        uint32_t longest = 0;
        for (uint32_t g = 0; g < n_graphs; ++g) {
            const uint32_t v0 = vertex_off[g], nv = vertex_off[g + 1] - v0, reg = g % n_regions, kk = k[g / n_regions];
            const uint32_t reads0 = region_read_off[reg], nr = region_read_off[reg + 1] - reads0;
            for (uint32_t v = 0; v < nv; ++v) {
                if (vertex_absent && vertex_absent[v0 + v]) continue;
                const auto vx = [&] { return "graph " + std::to_string(g) + ": vertex " + std::to_string(v) + ": "; };
                const uint32_t sq = vertex_seq[v0 + v], pos = vertex_pos[v0 + v];
                if (sq > nr) return fail(h, vx() + "its sequence " + std::to_string(sq) + " is not one of the region's (" + std::to_string(nr) + " reads)");
                uint32_t start, len;
                if (sq == 0) {
                    start = region_ref_off[reg];
                    len = region_ref_off[reg + 1] - start;
                } else {
                    const uint32_t r = reads0 + sq - 1;
                    start = n_ref + read_off[r] + (read_first ? read_first[r] : 0);
                    len = read_first ? read_len[r] : read_off[r + 1] - read_off[r];
                }
                if ((uint64_t)pos + kk > len) return fail(h, vx() + "its bytes [" + std::to_string(pos) + ", +" + std::to_string(kk) + ") leave their sequence (" + std::to_string(len) + " bases)");
                vertex_base[v0 + v] = start + pos;
            }
            for (uint32_t e = edge_off[g]; e < edge_off[g + 1]; ++e) {
                const auto ed = [&] { return "graph " + std::to_string(g) + ": edge " + std::to_string(e - edge_off[g]) + ": "; };
                if (edge_src[e] >= nv) return fail(h, ed() + "its source " + std::to_string(edge_src[e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (edge_dst[e] >= nv) return fail(h, ed() + "its target " + std::to_string(edge_dst[e]) + " reaches n_vertices (" + std::to_string(nv) + ")");
                if (edge_absent && edge_absent[e]) continue;
                if (vertex_absent && (vertex_absent[v0 + edge_src[e]] || vertex_absent[v0 + edge_dst[e]])) return fail(h, ed() + "it is present and an endpoint is absent");
                ++deg_out[v0 + edge_src[e]];
                ++deg_in[v0 + edge_dst[e]];
                if (edge_is_ref[e]) {  // (bit 0: a reference edge comes in, bit 1: one goes out)
                    ref_bits[v0 + edge_src[e]] |= 2;
                    ref_bits[v0 + edge_dst[e]] |= 1;
                }
            }
            uint64_t tails = 0, heads = 0;  // upper bounds: a merge gives no vertex a first in-edge that a later head list could miss
            for (uint32_t v = 0; v < nv; ++v) {
                if (vertex_absent && vertex_absent[v0 + v]) continue;
                // (out-degree 0 behind a reference edge is the reference sink, in-degree 0 in front of one the source: B:339-387.
                // Reference edges neither come nor go while the tails are taken, and the heads' list is made before a head is)
                tails += deg_out[v0 + v] == 0 && !(ref_bits[v0 + v] & 1);
                heads += deg_in[v0 + v] == 0 && !(ref_bits[v0 + v] & 2);
            }
            if (!(cfg.ops & PHMM_RECOVER_OP_TAILS)) tails = 0;
            if (!(cfg.ops & PHMM_RECOVER_OP_HEADS)) heads = 0;
            // a tail makes one edge; a head one edge and, extended, up to k vertices with an edge each
            const uint64_t xv = (uint64_t)xv_off[g] + nv + heads * kk, xe = (uint64_t)xe_off[g] + (edge_off[g + 1] - edge_off[g]) + tails + heads * (kk + 1ull);
            if (xv > 0xffffffffull || xe > 0xffffffffull) return fail(h, "graph " + std::to_string(g) + ": the working graph does not fit 32 bits");
            xv_off[g + 1] = (uint32_t)xv;
            xe_off[g + 1] = (uint32_t)xe;
            xend_off[g + 1] = xend_off[g] + (uint32_t)(tails + heads);
            if (tails + heads) longest = std::max(longest, nv);
        }
        const uint32_t slab_len = longest + k_max + 2;
        const int64_t w_max = std::max({std::abs((int64_t)cfg.sw_parameters.match_value), std::abs((int64_t)cfg.sw_parameters.mismatch_penalty),
                                        std::abs((int64_t)cfg.sw_parameters.gap_open_penalty), std::abs((int64_t)cfg.sw_parameters.gap_extend_penalty)});
        if (w_max * (2ll * slab_len + 2) >= 1000000000ll)
            return fail(h, "the Smith-Waterman weights times the longest strings reach 1e9: the reference's 32-bit sums overflow");
        const uint32_t XV = xv_off[n_graphs], XE = xe_off[n_graphs], XEND = xend_off[n_graphs], XNE = XE - E, XNV = XV - V;

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->recover_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the slots of the results; the working graphs and the slabs lie in the device-only workspace ----
        StageLayout L;
        const auto s_k = L.in(k, n_k);
        const auto s_vo = L.in(vertex_off, (size_t)n_graphs + 1), s_eo = L.in(edge_off, (size_t)n_graphs + 1);
        const auto s_rb = L.in(ref_bases, n_ref), s_qb = L.in(read_bases, n_read_bases);
        const auto s_vb = L.in(vertex_base.data(), V);
        const auto s_es = L.in(edge_src, E), s_ed = L.in(edge_dst, E), s_em = L.in(edge_multiplicity, E), s_ep = L.in(edge_pruning_multiplicity, E);
        const auto s_er = L.in(edge_is_ref, E);
        const auto s_va = L.in(vertex_absent, vertex_absent ? V : 0), s_ea = L.in(edge_absent, edge_absent ? E : 0);
        const auto s_pf = L.in(prune_factor, n_graphs);
        const auto s_xv = L.in(xv_off.data(), (size_t)n_graphs + 1), s_xe = L.in(xe_off.data(), (size_t)n_graphs + 1), s_xn = L.in(xend_off.data(), (size_t)n_graphs + 1);
        L.end_inputs();
        const auto o_counts = L.out<uint32_t>(8ull * n_graphs);
        const auto o_ev = L.out<uint32_t>(XEND), o_ek = L.out<uint32_t>(XEND), o_es = L.out<uint32_t>(XEND), o_ea = L.out<uint32_t>(XEND), o_er = L.out<uint32_t>(XEND),
                   o_en = L.out<uint32_t>(XEND), o_ec = L.out<uint32_t>((size_t)XEND * RECOVER_CIGAR_SHOWN), o_ee = L.out<uint32_t>(XEND);
        const auto o_ns = L.out<uint32_t>(XNE), o_nd = L.out<uint32_t>(XNE), o_nm = L.out<uint32_t>(XNE), o_np = L.out<uint32_t>(XNE);
        const auto o_nk = L.out<uint8_t>((size_t)XNV * k_max);
        const auto o_rm = L.out<uint8_t>(E);
        // (the vertex bases index one array: the reads' bases start where the reference's slot ends)
        const uint32_t read_base_shift = (uint32_t)(s_qb.off - s_rb.off) - n_ref;
        if (read_base_shift)
            for (uint32_t g = 0; g < n_graphs; ++g)
                for (uint32_t v = vertex_off[g]; v < vertex_off[g + 1]; ++v)
                    if (!(vertex_absent && vertex_absent[v]) && vertex_seq[v]) vertex_base[v] += read_base_shift;
        const size_t slab_bytes = recover_slab_bytes(slab_len);
        const uint32_t n_blocks = XEND ? (uint32_t)std::min<uint64_t>(std::min<uint32_t>(n_graphs, kMaxBlocks), std::max<uint64_t>(1, kSlabBudget / slab_bytes)) : std::min<uint32_t>(n_graphs, kMaxBlocks);
        StageLayout D;  // the device-only workspace: 41 bytes per vertex slot, 17 per edge slot, a slab per workgroup
        const auto w_xv = D.scratch<uint32_t>((size_t)RECOVER_VERTEX_WORDS * XV);
        const auto w_va = D.scratch<uint8_t>(XV);
        const auto w_es = D.scratch<uint32_t>(XE), w_ed = D.scratch<uint32_t>(XE), w_em = D.scratch<uint32_t>(XE), w_ep = D.scratch<uint32_t>(XE);
        const auto w_ef = D.scratch<uint8_t>(XE);
        const auto w_slab = D.scratch<unsigned char>(XEND ? slab_bytes * n_blocks : 0);
        if (!h->recover_scratch.reserve(h, D, "recovery workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "recovery staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->recover_scratch;

        RecoverParams p{};
        p.n_graphs = n_graphs;
        p.n_regions = n_regions;
        p.ops = cfg.ops;
        p.min_dangling_branch_length = cfg.min_dangling_branch_length;
        p.min_matching_bases = cfg.min_matching_bases;
        p.max_mismatches_in_dangling_head = cfg.max_mismatches_in_dangling_head;
        p.w_match = cfg.sw_parameters.match_value;
        p.w_mismatch = cfg.sw_parameters.mismatch_penalty;
        p.w_open = cfg.sw_parameters.gap_open_penalty;
        p.w_extend = cfg.sw_parameters.gap_extend_penalty;
        p.k = W.dev_ptr(s_k);
        p.vertex_off = W.dev_ptr(s_vo);
        p.edge_off = W.dev_ptr(s_eo);
        p.bases = W.dev_ptr(s_rb);
        p.vertex_base = W.dev_ptr(s_vb);
        p.edge_src = W.dev_ptr(s_es);
        p.edge_dst = W.dev_ptr(s_ed);
        p.edge_mult = W.dev_ptr(s_em);
        p.edge_pmult = W.dev_ptr(s_ep);
        p.edge_is_ref = W.dev_ptr(s_er);
        p.vertex_absent = vertex_absent ? W.dev_ptr(s_va) : nullptr;
        p.edge_absent = edge_absent ? W.dev_ptr(s_ea) : nullptr;
        p.prune_factor = W.dev_ptr(s_pf);
        p.xv_off = W.dev_ptr(s_xv);
        p.xe_off = W.dev_ptr(s_xe);
        p.xend_off = W.dev_ptr(s_xn);
        p.xv = ws.ptr(w_xv);
        p.xv_absent = ws.ptr(w_va);
        p.xe_src = ws.ptr(w_es);
        p.xe_dst = ws.ptr(w_ed);
        p.xe_mult = ws.ptr(w_em);
        p.xe_pmult = ws.ptr(w_ep);
        p.xe_flags = ws.ptr(w_ef);
        p.xv_total = XV;
        p.slab = ws.ptr(w_slab);
        p.slab_stride = slab_bytes;
        p.slab_len = slab_len;
        p.g_counts = W.dev_ptr(o_counts);
        p.end_vertex = W.dev_ptr(o_ev);
        p.end_kind = W.dev_ptr(o_ek);
        p.end_status = W.dev_ptr(o_es);
        p.end_alt_len = W.dev_ptr(o_ea);
        p.end_ref_len = W.dev_ptr(o_er);
        p.end_n_cigar = W.dev_ptr(o_en);
        p.end_cigar = W.dev_ptr(o_ec);
        p.end_edge = W.dev_ptr(o_ee);
        p.ne_src = W.dev_ptr(o_ns);
        p.ne_dst = W.dev_ptr(o_nd);
        p.ne_mult = W.dev_ptr(o_nm);
        p.ne_pmult = W.dev_ptr(o_np);
        p.new_kmer = W.dev_ptr(o_nk);
        p.kmer_stride = k_max;
        p.edge_removed = W.dev_ptr(o_rm);

        const auto launch = [&] {
            return (!o_nk.count || hip_ok(h, hipMemsetAsync(W.dev_ptr(o_nk), 0, o_nk.count, S), "memset(new k-mers)")) &&
                   hip_ok(h, launch_recover(p, n_blocks, S), "recovery kernel");
        };
        if (!stage_round_trip(h, W, L, S, "recovery", launch)) return PHMM_ERR_HIP;

        // ---- the sizes; then, if everything fits, the slots cut down to what was made --------------------------------------------
        const uint32_t *counts = W.host_ptr(o_counts);
        uint64_t need[3] = {0, 0, 0};
        for (uint32_t g = 0; g < n_graphs; ++g) {
            need[0] += counts[8ull * g + 7];
            need[1] += counts[8ull * g + 4];
            need[2] += counts[8ull * g + 5];
        }
        const bool fits = need[0] <= capacity[0] && need[1] <= capacity[1] && need[2] <= capacity[2];
        const bool null_array = (need[0] && (!end_vertex || !end_kind || !end_status || !end_alt_len || !end_ref_len || !end_n_cigar || !end_cigar || !end_edge)) ||
                                (need[1] && (!new_edge_src || !new_edge_dst || !new_edge_multiplicity || !new_edge_pruning_multiplicity)) ||
                                (need[2] && !new_vertex_kmer);
        if (fits && null_array) return fail(h, "a capacity above 0 whose arrays are NULL");
        for (int i = 0; i < 3; ++i) required[i] = (uint32_t)need[i];
        if (!fits) {
            h->err = "phmm_assembly_recover: an output array is too small (required holds the sizes)";
            return h->err_code = PHMM_ERR_EVENT_CAPACITY;
        }
        uint32_t at_end = 0, at_edge = 0, at_vertex = 0;
        uint32_t *const per_graph[7] = {n_tails, n_tails_recovered, n_heads, n_heads_recovered, n_new_edges, n_new_vertices, n_rounds};
        for (uint32_t g = 0; g < n_graphs; ++g) {
            const uint32_t *c = counts + 8ull * g;
            for (int i = 0; i < 7; ++i) per_graph[i][g] = c[i];
            end_off[g] = at_end;
            new_edge_off[g] = at_edge;
            new_vertex_off[g] = at_vertex;
            const uint32_t e_from = xend_off[g], ne_from = xe_off[g] - edge_off[g], nv_from = xv_off[g] - vertex_off[g];
            if (c[7]) {
                const auto cut = [&](uint32_t *dst, StageSlot<uint32_t> s, size_t width) { memcpy(dst + (size_t)at_end * width, W.host_ptr(s) + (size_t)e_from * width, 4 * width * c[7]); };
                cut(end_vertex, o_ev, 1);
                cut(end_kind, o_ek, 1);
                cut(end_status, o_es, 1);
                cut(end_alt_len, o_ea, 1);
                cut(end_ref_len, o_er, 1);
                cut(end_n_cigar, o_en, 1);
                cut(end_cigar, o_ec, RECOVER_CIGAR_SHOWN);
                cut(end_edge, o_ee, 1);
            }
            if (c[4]) {
                memcpy(new_edge_src + at_edge, W.host_ptr(o_ns) + ne_from, 4ull * c[4]);
                memcpy(new_edge_dst + at_edge, W.host_ptr(o_nd) + ne_from, 4ull * c[4]);
                memcpy(new_edge_multiplicity + at_edge, W.host_ptr(o_nm) + ne_from, 4ull * c[4]);
                memcpy(new_edge_pruning_multiplicity + at_edge, W.host_ptr(o_np) + ne_from, 4ull * c[4]);
            }
            if (c[5]) memcpy(new_vertex_kmer + (size_t)at_vertex * k_max, W.host_ptr(o_nk) + (size_t)nv_from * k_max, (size_t)c[5] * k_max);
            at_end += c[7];
            at_edge += c[4];
            at_vertex += c[5];
        }
        end_off[n_graphs] = at_end;
        new_edge_off[n_graphs] = at_edge;
        new_vertex_off[n_graphs] = at_vertex;
        if (E) memcpy(edge_removed, W.host_ptr(o_rm), E);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_recover", PHMM_FAIL_CODE)
}
