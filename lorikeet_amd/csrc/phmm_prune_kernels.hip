// phmm_assembly_prune (include/phmm.h): what the assembler does to the raw read-threading graph before it looks for paths --
// low-weight chains (chain_pruner.rs:39-118, low_weight_chain_pruner.rs:24-36), orphans (base_graph.rs:392-406), the cycle
// verdict (base_graph.rs:615-617), the reference ends (base_graph.rs:339-428), the vertices dangling-end recovery starts from
// (read_threading_graph.rs:792-797, 837-842) and remove_paths_not_connected_to_ref (base_graph.rs:626-656).
//
// One workgroup per graph, one kernel, passes separated by workgroup barriers; everything is integers, bytes and atomics.  The
// reference states each step serially (a deque, a DFS, a heap); none of the results depends on that order:
//   chains    an edge's head is the edge itself if its source is not interior (in-degree 1 and out-degree 1), else the head
//             of the source's one in-edge: pointer jumping over e_ptr.  A half-updated pointer is still an ancestor, so the
//             jumps run in place.  An edge that has met no head after ceil(log2(edges + 1)) + 1 rounds lies on a ring.
//   found     find_all_chains reaches a head exactly when its source can be reached from a vertex of in-degree 0.
//   cycle     Kahn's peeling: what cannot be peeled lies on or behind a cycle.
// Every sweep (reachability, peeling) relaxes edges until a round changes nothing and is bounded by vertices + 1 rounds.  A
// thread sweeps a contiguous run of edges, ascending forwards and descending backwards: phmm_assembly_graph numbers edges in
// threading order, so a run carries a mark along a whole stretch of a path in one round.
#include "phmm_prune_internal.hpp"

namespace phmm {
namespace {

constexpr uint8_t E_HEAD = 1, E_KEEP = 2, E_PEELED = 4;
constexpr uint8_t GONE = PRUNE_ABSENT | PRUNE_REMOVED_CHAINS | PRUNE_REMOVED_CONNECT;
enum { S_NV0, S_CHAINS, S_REMOVED, S_ORPHANS, S_FLAGS, S_VLEFT, S_ELEFT, S_SOURCE, S_SINK, S_COUNT };

__global__ __launch_bounds__(PRUNE_THREADS) void prune_kernel(PruneParams p) {
    const uint32_t g = blockIdx.x, tid = threadIdx.x, T = PRUNE_THREADS;
    const uint32_t v0 = p.vertex_off[g], nv = p.vertex_off[g + 1] - v0, e0 = p.edge_off[g], ne = p.edge_off[g + 1] - e0;
    const uint32_t *const src = p.edge_src + e0, *const dst = p.edge_dst + e0, *const mult = p.edge_mult + e0;
    const uint8_t *const is_ref = p.edge_is_ref + e0;
    const uint8_t *const v_absent = p.vertex_absent ? p.vertex_absent + v0 : nullptr, *const e_absent = p.edge_absent ? p.edge_absent + e0 : nullptr;
    uint32_t *const v_in = p.v_in + v0, *const v_out = p.v_out + v0, *const v_inedge = p.v_inedge + v0, *const v_ref = p.v_ref + v0, *const v_mark = p.v_mark + v0;
    uint32_t *const e_ptr = p.e_ptr + e0, *const chain = p.edge_chain + e0;
    uint8_t *const e_bits = p.e_bits + e0, *const e_state = p.edge_state + e0, *const v_state = p.vertex_state + v0;
    const bool chains = p.ops & PRUNE_OP_CHAINS, connect = p.ops & PRUNE_OP_CONNECT;
    const uint32_t factor = p.prune_factor[g];
    // a thread's contiguous run of edges, for the sweeps
    const uint32_t per = ne / T + (ne % T != 0);  // (tid x per < 2^32: per <= 2^24)
    const uint32_t lo = tid * per < ne ? tid * per : ne, hi = ne - lo < per ? ne : lo + per;
    const uint32_t max_rounds = nv + 1;

    __shared__ uint32_t s[S_COUNT];
    if (tid < S_COUNT) s[tid] = tid >= S_SOURCE ? PRUNE_NONE : 0;
    __syncthreads();

    // ---- G0: the input without the absent elements ------------------------------------------------------------------------
    uint32_t n = 0;
    for (uint32_t v = tid; v < nv; v += T) {
        const bool absent = v_absent && v_absent[v];
        v_state[v] = absent ? PRUNE_ABSENT : 0;
        v_in[v] = v_out[v] = v_ref[v] = v_mark[v] = 0;
        n += !absent;
    }
    if (n) atomicAdd(&s[S_NV0], n);
    for (uint32_t e = tid; e < ne; e += T) {
        e_state[e] = e_absent && e_absent[e] ? PRUNE_ABSENT : 0;
        e_bits[e] = 0;
        chain[e] = PRUNE_NONE;
    }
    __syncthreads();
    const uint32_t nv0 = s[S_NV0];

    if (chains) {
        for (uint32_t e = tid; e < ne; e += T) {
            if (e_state[e]) continue;
            atomicAdd(&v_out[src[e]], 1u);
            atomicAdd(&v_in[dst[e]], 1u);
            v_inedge[dst[e]] = e;
        }
        __syncthreads();
        // heads, and the vertices find_all_chains starts from (C:61)
        for (uint32_t e = tid; e < ne; e += T) {
            if (e_state[e]) continue;
            const uint32_t a = src[e];
            if (v_in[a] == 1 && v_out[a] == 1) {
                e_ptr[e] = v_inedge[a];
            } else {
                e_ptr[e] = e;
                e_bits[e] = E_HEAD;
            }
        }
        for (uint32_t v = tid; v < nv; v += T)
            if (!v_state[v] && !v_in[v]) v_mark[v] = 1;
        __syncthreads();
        const int jumps = (ne ? 32 - __clz(ne) : 0) + 2;  // >= ceil(log2(edges + 1)) + 1
        for (int r = 0; r < jumps; ++r) {
            int changed = 0;
            for (uint32_t e = tid; e < ne; e += T) {
                if (e_state[e]) continue;
                const uint32_t q = e_ptr[e], qq = e_ptr[q];
                if (qq != q) {
                    e_ptr[e] = qq;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        // what the sources reach (C:67-78)
        for (uint32_t r = 0; r < max_rounds; ++r) {
            int changed = 0;
            for (uint32_t e = lo; e < hi; ++e) {
                if (e_state[e]) continue;
                if (v_mark[src[e]] && !v_mark[dst[e]]) {
                    v_mark[dst[e]] = 1;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        // an edge of weight >= the factor, or a reference edge, protects its chain (L:24-36)
        for (uint32_t e = tid; e < ne; e += T) {
            if (e_state[e]) continue;
            const uint32_t h = e_ptr[e];
            if ((e_bits[h] & E_HEAD) && (is_ref[e] || mult[e] >= factor)) e_bits[h] = E_HEAD | E_KEEP;
        }
        __syncthreads();
        uint32_t n_found = 0, n_removed = 0;
        for (uint32_t e = tid; e < ne; e += T) {
            if (e_state[e]) continue;
            const uint32_t h = e_ptr[e];
            const uint8_t hb = e_bits[h];
            if (!(hb & E_HEAD) || !v_mark[src[h]]) continue;  // a ring, or a chain no source reaches
            chain[e] = h;
            n_found += e == h;
            if (!(hb & E_KEEP)) {
                e_state[e] = PRUNE_REMOVED_CHAINS;
                n_removed += e == h;
            }
        }
        if (n_found) atomicAdd(&s[S_CHAINS], n_found);
        if (n_removed) atomicAdd(&s[S_REMOVED], n_removed);
        __syncthreads();
        for (uint32_t v = tid; v < nv; v += T) v_in[v] = v_out[v] = v_mark[v] = 0;
        __syncthreads();
    }

    // ---- G1: degrees, orphans (B:392-406), the reference ends, the dangling ends ---------------------------------------------
    for (uint32_t e = tid; e < ne; e += T) {
        if (e_state[e]) continue;
        atomicAdd(&v_out[src[e]], 1u);
        atomicAdd(&v_in[dst[e]], 1u);
        if (is_ref[e]) {
            atomicOr(&v_ref[src[e]], 2u);
            atomicOr(&v_ref[dst[e]], 1u);
        }
    }
    __syncthreads();
    if (chains && nv0 != 1) {  // (an orphan is no ref source unless it is the graph's only vertex: B:359)
        n = 0;
        for (uint32_t v = tid; v < nv; v += T)
            if (!v_state[v] && !v_in[v] && !v_out[v]) {
                v_state[v] = PRUNE_REMOVED_CHAINS;
                ++n;
            }
        if (n) atomicAdd(&s[S_ORPHANS], n);
    }
    __syncthreads();
    const uint32_t nv1 = nv0 - s[S_ORPHANS];
    for (uint32_t v = tid; v < nv; v += T) {
        if (v_state[v]) continue;
        const uint32_t r = v_ref[v];
        const bool source = !(r & 1) && ((r & 2) || nv1 == 1), sink = !(r & 2) && ((r & 1) || nv1 == 1);  // B:339-387
        if (source) atomicMin(&s[S_SOURCE], v);
        if (sink) atomicMin(&s[S_SINK], v);
        v_state[v] = (!v_out[v] && !sink ? PRUNE_DANGLING_TAIL : 0) | (!v_in[v] && !source ? PRUNE_DANGLING_HEAD : 0);
        if (!v_in[v]) v_mark[v] = 1;  // peeled
    }
    __syncthreads();
    // ---- the cycle verdict: peel vertices without an unpeeled in-edge ---------------------------------------------------------
    for (uint32_t r = 0; r < max_rounds; ++r) {
        int changed = 0;
        for (uint32_t e = lo; e < hi; ++e) {
            if (e_state[e] || (e_bits[e] & E_PEELED) || !v_mark[src[e]]) continue;
            e_bits[e] |= E_PEELED;
            if (atomicSub(&v_in[dst[e]], 1u) == 1) {
                v_mark[dst[e]] = 1;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    n = 0;
    for (uint32_t v = tid; v < nv; v += T) n |= !(v_state[v] & GONE) && !v_mark[v];
    if (n) atomicOr(&s[S_FLAGS], PRUNE_HAS_CYCLE);
    __syncthreads();
    const uint32_t source = s[S_SOURCE], sink = s[S_SINK];
    const bool ends = source != PRUNE_NONE && sink != PRUNE_NONE;

    // ---- G2: what lies on a way from the reference source to the reference sink (B:626-656) ---------------------------------
    if (connect && ends) {
        for (uint32_t v = tid; v < nv; v += T) v_mark[v] = (v == source ? 1 : 0) | (v == sink ? 2 : 0);
        __syncthreads();
        for (uint32_t r = 0; r < max_rounds; ++r) {  // forwards: only bit 0 changes
            int changed = 0;
            for (uint32_t e = lo; e < hi; ++e) {
                if (e_state[e]) continue;
                const uint32_t m = v_mark[dst[e]];
                if ((v_mark[src[e]] & 1) && !(m & 1)) {
                    v_mark[dst[e]] = m | 1;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (uint32_t r = 0; r < max_rounds; ++r) {  // backwards: only bit 1 changes
            int changed = 0;
            for (uint32_t e = hi; e-- > lo;) {
                if (e_state[e]) continue;
                const uint32_t m = v_mark[src[e]];
                if ((v_mark[dst[e]] & 2) && !(m & 2)) {
                    v_mark[src[e]] = m | 2;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (uint32_t v = tid; v < nv; v += T)
            if (!(v_state[v] & GONE) && v_mark[v] != 3) v_state[v] |= PRUNE_REMOVED_CONNECT;
        __syncthreads();
        for (uint32_t e = tid; e < ne; e += T)
            if (!e_state[e] && ((v_state[src[e]] | v_state[dst[e]]) & PRUNE_REMOVED_CONNECT)) e_state[e] = PRUNE_REMOVED_CONNECT;
    }
    uint32_t n_v = 0, n_e = 0;
    for (uint32_t v = tid; v < nv; v += T) n_v += !(v_state[v] & GONE);
    for (uint32_t e = tid; e < ne; e += T) n_e += !e_state[e];
    if (n_v) atomicAdd(&s[S_VLEFT], n_v);
    if (n_e) atomicAdd(&s[S_ELEFT], n_e);
    __syncthreads();
    if (tid == 0) {
        p.graph_flags[g] = s[S_FLAGS] | (ends ? 0 : PRUNE_NO_REF_ENDS);
        p.n_chains[g] = s[S_CHAINS];
        p.n_chains_removed[g] = s[S_REMOVED];
        p.n_vertices_left[g] = s[S_VLEFT];
        p.n_edges_left[g] = s[S_ELEFT];
        p.ref_source[g] = source;
        p.ref_sink[g] = sink;
    }
}

}  // namespace

hipError_t launch_prune(const PruneParams &p, hipStream_t stream) {
    if (!p.n_graphs) return hipSuccess;
    hipLaunchKernelGGL(prune_kernel, dim3(p.n_graphs), dim3(PRUNE_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
