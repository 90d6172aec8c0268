// The k best haplotype paths of many sequence graphs (phmm_assembly_best_paths): what the reference's
// GraphBasedKBestHaplotypeFinder does -- the cycle removal of its constructor as written, then the best-first search -- one wave
// per graph, then the offsets of all graphs, the paths' edges and bytes at those offsets, and the duplicate marks.  Every loop
// ends at a bound computed from the sizes of the graph at hand.  Scores: parent + (L[m] - L[T]) from the handle's table of the
// host library's log10, two roundings and no multiply, so nothing can contract.
#include "phmm_paths_internal.hpp"

namespace phmm {
namespace {

using u64 = uint64_t;

__device__ inline u64 lanes_below() { return (1ull << (threadIdx.x & 63)) - 1; }
__device__ inline uint32_t rank_in(u64 mask) { return (uint32_t)__popcll(mask & lanes_below()); }
__device__ inline u64 shfl64(u64 x, int src) {
    const uint32_t lo = __shfl((uint32_t)x, src), hi = __shfl((uint32_t)(x >> 32), src);
    return (u64)hi << 32 | lo;
}
__device__ inline u64 shfl_xor64(u64 x, int mask) {
    const uint32_t lo = __shfl_xor((uint32_t)x, mask), hi = __shfl_xor((uint32_t)(x >> 32), mask);
    return (u64)hi << 32 | lo;
}
__device__ inline u64 shfl_up64(u64 x, int delta) {
    const uint32_t lo = __shfl_up((uint32_t)x, delta), hi = __shfl_up((uint32_t)(x >> 32), delta);
    return (u64)hi << 32 | lo;
}
__device__ inline u64 wave_sum(u64 x) {
    for (int o = 32; o; o >>= 1) x += shfl_xor64(x, o);
    return x;
}
__device__ inline u64 wave_inclusive_scan(u64 x) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = shfl_up64(x, o);
        if (lane >= o) x += y;
    }
    return x;
}
__device__ inline uint32_t saturate32(u64 x) { return x > 0xffffffffull ? 0xffffffffu : (uint32_t)x; }

// OrderedFloat's order as an unsigned key: NaN is greatest and equal to itself, -0.0 equals 0.0
__device__ inline u64 score_key(double s) {
    if (s != s) return ~0ull;
    if (s == 0.0) s = 0.0;
    const u64 b = (u64)__double_as_longlong(s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// one graph as its wave sees it
struct Graph {
    uint32_t v0, nv, e0, ne, b0, nb;
    const uint32_t *vbo, *src, *dst, *mult;
    const uint8_t *role;
    uint32_t source, sink;
    __device__ bool is_source(uint32_t v) const { return role ? (role[v] & 1) != 0 : v == source; }
    __device__ bool is_sink(uint32_t v) const { return role ? (role[v] & 2) != 0 : v == sink; }
    __device__ uint32_t vlen(uint32_t v) const { return (v + 1 < nv ? vbo[v + 1] : nb) - vbo[v]; }
};
__device__ inline Graph load_graph(const PathsParams &p, uint32_t g) {
    Graph G;
    G.v0 = p.vertex_off[g], G.nv = p.vertex_off[g + 1] - G.v0;
    G.e0 = p.edge_off[g], G.ne = p.edge_off[g + 1] - G.e0;
    G.b0 = p.base_off[g], G.nb = p.base_off[g + 1] - G.b0;
    G.vbo = p.vertex_base_off + G.v0;
    G.src = p.edge_src + G.e0, G.dst = p.edge_dst + G.e0, G.mult = p.edge_mult + G.e0;
    G.role = p.vertex_role ? p.vertex_role + G.v0 : nullptr;
    G.source = p.vertex_role ? PATHS_NONE : p.graph_source[g];
    G.sink = p.vertex_role ? PATHS_NONE : p.graph_sink[g];
    return G;
}

// the search tree of one graph
struct Tree {
    uint32_t *parent, *edge, *vertex, *len, *bytes;
    double *score;
    uint8_t *is_ref;
};

// KBestHaplotype::cmp behind equal scores (k_best_haplotype.rs:103-112): the path with the lexicographically smaller edge list
// is the greater, a proper prefix before its extension.  Both paths are root-to-node paths of one forest, so their lists
// first differ behind their lowest common ancestor, where two children of one node hold different edges; without one (two
// sources) they differ at position 0, and two zero-edge paths go by the vertex (the contract).  At most len(a) + len(b) steps.
__device__ bool path_before(const Tree &t, uint32_t a, uint32_t b) {
    const uint32_t la = t.len[a], lb = t.len[b];
    uint32_t x = a, y = b;
    for (uint32_t i = lb; i < la; ++i) x = t.parent[x];
    for (uint32_t i = la; i < lb; ++i) y = t.parent[y];
    if (x == y) return la < lb;
    uint32_t d = la < lb ? la : lb;
    for (; d > 1 && t.parent[x] != t.parent[y]; --d) x = t.parent[x], y = t.parent[y];
    if (d == 0) return la != lb ? la < lb : t.vertex[x] < t.vertex[y];
    return t.edge[x] < t.edge[y];
}
__device__ inline bool entry_before(const Tree &t, u64 ka, uint32_t na, u64 kb, uint32_t nb) {
    return ka != kb ? ka > kb : path_before(t, na, nb);
}

// ---- the search: one wave per graph ----------------------------------------------------------------------------------------------
// The hand-overs between lanes through the workspace and the peel's s_tail are ordered by __syncthreads() alone because the
// workgroup is exactly one wave, which runs in lockstep: a larger block would make them races.
static_assert(PATHS_THREADS == 64, "paths_search_kernel is written for a workgroup of one wave");
__global__ __launch_bounds__(PATHS_THREADS) void paths_search_kernel(PathsParams p) {
    __shared__ uint32_t s_tail;
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const Graph G = load_graph(p, g);
    const uint32_t nv = G.nv, ne = G.ne;
    const size_t row = (size_t)G.v0 + g;  // the graph's rows in the vertex planes: one element more than vertices
    uint32_t *const out = p.w + PATHS_V_OUT * p.w_stride + row, *const fill = p.w + PATHS_V_FILL * p.w_stride + row;
    uint32_t *const list = p.w + PATHS_V_LIST * p.w_stride + row, *const cursor = p.w + PATHS_V_CURSOR * p.w_stride + row;
    uint32_t *const seen = p.w + PATHS_V_SEEN * p.w_stride + row;
    uint32_t *const csr = p.e_csr + G.e0;
    uint8_t *const e_gone = p.edge_removed + G.e0, *const v_gone = p.vertex_removed + G.v0, *const reach = p.stack_reach + G.v0;
    uint32_t status = p.pre_status[g];
    uint32_t n_res = 0, n_popped = 0, n_edges_gone = 0, n_vertices_gone = 0;
    u64 sum_edges = 0, sum_bytes = 0;

    for (uint32_t i = lane; i < ne; i += 64) e_gone[i] = 0;
    for (uint32_t i = lane; i < nv; i += 64) v_gone[i] = 0;
    if (status == PATHS_OK) {
        // (a) the out-edges of every vertex, descending: count, scan, place, sort
        for (uint32_t i = lane; i <= nv; i += 64) fill[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < ne; i += 64) atomicAdd(&fill[G.src[i]], 1u);
        __syncthreads();
        uint32_t run = 0;
        for (uint32_t base = 0; base < nv; base += 64) {
            const uint32_t i = base + lane, c = i < nv ? fill[i] : 0;
            const uint32_t incl = (uint32_t)wave_inclusive_scan(c);
            if (i < nv) out[i] = run + incl - c;
            run += __shfl(incl, 63);
        }
        if (lane == 0) out[nv] = run;
        __syncthreads();
        for (uint32_t i = lane; i < nv; i += 64) fill[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < ne; i += 64) {
            const uint32_t s = G.src[i];
            csr[out[s] + atomicAdd(&fill[s], 1u)] = i;
        }
        __syncthreads();
        for (uint32_t v = lane; v < nv; v += 64) {  // a lane sorts its vertex's list (insertion: the lists are short)
            const uint32_t a = out[v], b = out[v + 1];
            for (uint32_t i = a + 1; i < b; ++i) {
                const uint32_t x = csr[i];
                uint32_t j = i;
                for (; j > a && csr[j - 1] < x; --j) csr[j] = csr[j - 1];
                csr[j] = x;
            }
        }
        __syncthreads();

        // (b) is_cyclic_directed over the whole graph: peel the vertices of in-degree 0 from a worklist
        for (uint32_t i = lane; i < nv; i += 64) fill[i] = 0, seen[i] = 0;
        __syncthreads();
        for (uint32_t i = lane; i < ne; i += 64) atomicAdd(&fill[G.dst[i]], 1u);
        __syncthreads();
        uint32_t tail = 0, head = 0;
        for (uint32_t base = 0; base < nv; base += 64) {
            const uint32_t i = base + lane;
            const bool z = i < nv && fill[i] == 0;
            const u64 m = __ballot(z);
            if (z) list[tail + rank_in(m)] = i;
            tail += (uint32_t)__popcll(m);
        }
        if (lane == 0) s_tail = tail;
        __syncthreads();
        for (uint32_t it = 0; it < nv && head < tail; ++it) {  // every round takes at least one vertex
            const uint32_t n = tail - head < 64 ? tail - head : 64;
            if (lane < n) {
                const uint32_t v = list[head + lane];
                for (uint32_t j = out[v]; j < out[v + 1]; ++j) {
                    const uint32_t d = G.dst[csr[j]];
                    if (atomicSub(&fill[d], 1u) == 1) list[atomicAdd(&s_tail, 1u)] = d;  // each vertex reaches 0 once: at most nv entries
                }
            }
            head += n;
            __syncthreads();
            tail = s_tail;
        }
        const bool cyclic = tail < nv;
        __syncthreads();

        // (c) remove_cycles_and_vertices_that_dont_lead_to_sinks as written (k_best_haplotype_finder.rs:87-182): a serial walk
        if (cyclic) {
            uint32_t found = 0;
            if (lane == 0) {
                const uint32_t first = G.role ? 0 : G.source, last = G.role ? nv : G.source + 1;
                const u64 bound = (u64)ne + 2ull * nv + 2;  // every step moves a cursor, pushes or pops
                uint32_t ord = 0;
                for (uint32_t sv = first; sv < last; ++sv) {
                    if (!G.is_source(sv)) continue;
                    ++ord;  // a fresh parent_vertices per source
                    if (G.is_sink(sv)) {
                        found = 1;
                        continue;
                    }
                    uint32_t depth = 1;
                    list[0] = sv, cursor[0] = out[sv], reach[0] = 0, seen[sv] = ord;
                    for (u64 step = 0; depth && step < bound; ++step) {
                        const uint32_t t = depth - 1, v = list[t], at = cursor[t];
                        if (at < out[v + 1]) {
                            cursor[t] = at + 1;
                            const uint32_t e = csr[at], c = G.dst[e];
                            if (seen[c] == ord) {
                                e_gone[e] = 1;  // an edge to any visited vertex: parent_vertices is never shrunk
                            } else if (G.is_sink(c)) {
                                reach[t] = 1;  // a sink returns true at once, unmarked and unexplored
                            } else {
                                seen[c] = ord, list[depth] = c, cursor[depth] = out[c], reach[depth] = 0;
                                ++depth;  // at most nv: every push marks a new vertex
                            }
                        } else {
                            const uint8_t r = reach[t];
                            if (!r) v_gone[v] = 1;
                            if (--depth) {
                                if (r) reach[depth - 1] = 1;
                            } else {
                                found |= r;
                            }
                        }
                    }
                }
            }
            __syncthreads();
            found = __shfl(found, 0);
            uint32_t marks = 0;
            for (uint32_t base = 0; base < ne; base += 64) marks += (uint32_t)__popcll(__ballot(base + lane < ne && e_gone[base + lane]));
            for (uint32_t base = 0; base < nv; base += 64) {
                const uint32_t c = (uint32_t)__popcll(__ballot(base + lane < nv && v_gone[base + lane]));
                marks += c, n_vertices_gone += c;
            }
            if (!found) status = PATHS_NO_PATH;
            else if (!marks) status = PATHS_CYCLES_STAY;
            if (status != PATHS_OK) {  // the reference panics: the graph is as it came
                for (uint32_t i = lane; i < ne; i += 64) e_gone[i] = 0;
                for (uint32_t i = lane; i < nv; i += 64) v_gone[i] = 0;
                n_vertices_gone = 0;
            } else {  // remove_all_vertices takes the vertices' edges along
                for (uint32_t base = 0; base < ne; base += 64) {
                    const uint32_t i = base + lane;
                    uint8_t m = 0;
                    if (i < ne) {
                        m = e_gone[i] | (uint8_t)((v_gone[G.src[i]] | v_gone[G.dst[i]]) << 1);
                        e_gone[i] = m;
                    }
                    n_edges_gone += (uint32_t)__popcll(__ballot(m != 0));
                }
            }
            __syncthreads();
        }
    }

    if (status == PATHS_OK) {
        // (d) find_best_haplotypes (graph_based_k_best_haplotype_finder.rs:64-132)
        const u64 nb = p.node_off[g];
        const uint32_t pool = (uint32_t)(p.node_off[g + 1] - nb), K = p.max_paths;
        const bool unlimited = K == 0xffffffffu;
        Tree t{p.n_parent + nb, p.n_edge + nb, p.n_vertex + nb, p.n_len + nb, p.n_bytes + nb, p.n_score + nb, p.n_is_ref + nb};
        u64 *const q_key = p.q_key + nb;
        uint32_t *const q_node = p.q_node + nb, *const r_node = p.r_node + nb;
        uint32_t n_nodes = 0, qn = 0;
        for (uint32_t i = lane; i < nv; i += 64) fill[i] = 0;  // vertex_counts
        for (uint32_t base = 0; base < nv && status == PATHS_OK; base += 64) {  // the sources, ascending
            const uint32_t v = base + lane;
            const bool s = v < nv && G.is_source(v);
            const u64 m = __ballot(s);
            const uint32_t c = (uint32_t)__popcll(m);
            if (c > pool - n_nodes) {
                status = PATHS_BUDGET;
                break;
            }
            if (s) {
                const uint32_t n = n_nodes + rank_in(m);
                t.parent[n] = PATHS_NONE, t.edge[n] = PATHS_NONE, t.vertex[n] = v, t.len[n] = 0, t.bytes[n] = G.vlen(v);
                t.score[n] = 0.0, t.is_ref[n] = 1;
                q_key[n] = score_key(0.0), q_node[n] = n;
            }
            n_nodes += c, qn += c;
        }
        __syncthreads();
        for (uint32_t it = 0; it < pool && qn && (unlimited || n_res < K) && status == PATHS_OK; ++it) {  // a node pops once
            // BinaryHeap::pop: the greatest entry, whatever the heap's shape -- no two entries compare equal
            bool have = false;
            u64 bk = 0;
            uint32_t bn = 0, bi = 0;
            for (uint32_t i = lane; i < qn; i += 64) {
                const u64 k = q_key[i];
                const uint32_t n = q_node[i];
                if (!have || entry_before(t, k, n, bk, bn)) have = true, bk = k, bn = n, bi = i;
            }
            for (int o = 32; o; o >>= 1) {
                const bool have2 = __shfl_xor((int)have, o) != 0;
                const u64 k2 = shfl_xor64(bk, o);
                const uint32_t n2 = __shfl_xor(bn, o), i2 = __shfl_xor(bi, o);
                if (have2 && (!have || (n2 != bn && entry_before(t, k2, n2, bk, bn)))) have = true, bk = k2, bn = n2, bi = i2;
            }
            bn = __shfl(bn, 0), bi = __shfl(bi, 0);
            __syncthreads();
            if (lane == 0) q_key[bi] = q_key[qn - 1], q_node[bi] = q_node[qn - 1];
            --qn, ++n_popped;
            __syncthreads();  // the children below take the slot that entry left
            const uint32_t v = t.vertex[bn];
            if (G.is_sink(v)) {
                if (lane == 0) r_node[n_res] = bn;
                ++n_res;
            } else if (!v_gone[v]) {  // vertex_counts holds the vertices of the graph behind the removal
                uint32_t count = 0;
                if (lane == 0) count = fill[v] = fill[v] + 1;
                count = __shfl(count, 0);
                if (unlimited || count < K) {
                    const uint32_t a = out[v], b = out[v + 1], len = t.len[bn] + 1;
                    u64 total = 0;
                    for (uint32_t j = a + lane; j < b; j += 64) total += e_gone[csr[j]] ? 0 : G.mult[csr[j]];
                    total = wave_sum(total);
                    const double s0 = t.score[bn], lt = p.log10_table[total];
                    const uint8_t r0 = t.is_ref[bn];
                    const uint32_t by0 = t.bytes[bn];
                    if (len > nv) status = PATHS_BUDGET;  // (a path visits a vertex once: cannot happen)
                    for (uint32_t base = a; base < b && status == PATHS_OK; base += 64) {
                        const uint32_t j = base + lane, e = j < b ? csr[j] : 0;
                        const bool present = j < b && !e_gone[e];
                        const u64 m = __ballot(present);
                        const uint32_t c = (uint32_t)__popcll(m);
                        if (c > pool - n_nodes) {
                            status = PATHS_BUDGET;
                            break;
                        }
                        if (present) {
                            const uint32_t n = n_nodes + rank_in(m), d = G.dst[e];
                            double s = s0 + (p.log10_table[G.mult[e]] - lt);
                            if (s != s) s = __longlong_as_double(0x7ff8000000000000ll);  // one NaN, whatever the sign the subtraction gave it
                            t.parent[n] = bn, t.edge[n] = e, t.vertex[n] = d, t.len[n] = len, t.bytes[n] = by0 + G.vlen(d);
                            t.score[n] = s, t.is_ref[n] = r0 & (p.edge_is_ref[G.e0 + e] != 0);
                            const uint32_t q = qn + rank_in(m);
                            q_key[q] = score_key(s), q_node[q] = n;
                        }
                        n_nodes += c, qn += c;
                    }
                }
            }
            __syncthreads();
        }
        if (status == PATHS_OK) {
            for (uint32_t r = lane; r < n_res; r += 64) sum_edges += t.len[r_node[r]], sum_bytes += t.bytes[r_node[r]];
            sum_edges = wave_sum(sum_edges), sum_bytes = wave_sum(sum_bytes);
        } else {
            n_res = 0;
        }
    }
    if (lane == 0) {
        uint32_t *c = p.g_counts + (size_t)PATHS_COUNTS * g;
        c[PATHS_C_STATUS] = status, c[PATHS_C_PATHS] = n_res, c[PATHS_C_POPPED] = n_popped;
        c[PATHS_C_EDGES_REMOVED] = n_edges_gone, c[PATHS_C_VERTICES_REMOVED] = n_vertices_gone;
        c[PATHS_C_PATH_EDGES] = saturate32(sum_edges), c[PATHS_C_HAP_BYTES] = saturate32(sum_bytes);
    }
}

// ---- where every graph's paths, path edges and bytes start; whether the caller's arrays hold them ---------------------------------
__global__ __launch_bounds__(64) void paths_offsets_kernel(PathsParams p) {
    const uint32_t lane = threadIdx.x, n = p.n_graphs;
    const int which[3] = {PATHS_C_PATHS, PATHS_C_PATH_EDGES, PATHS_C_HAP_BYTES};
    bool fits = true, overflow = false;
    for (int k = 0; k < 3; ++k) {
        uint32_t *const off = p.out_off + (size_t)k * (n + 1);
        u64 run = 0;
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            const u64 c = i < n ? p.g_counts[(size_t)PATHS_COUNTS * i + which[k]] : 0;
            overflow = overflow || __any(c == 0xffffffffull);  // a graph's own count was saturated
            const u64 incl = wave_inclusive_scan(c);
            if (i < n) off[i] = saturate32(run + incl - c);
            run += shfl64(incl, 63);
        }
        if (lane == 0) off[n] = saturate32(run);
        fits = fits && run <= p.capacity[k];
        overflow = overflow || run >= 0xffffffffull;
    }
    if (lane == 0) *p.fits = overflow ? PATHS_FITS_OVERFLOW : fits;  // (the later kernels run only on PATHS_FITS_YES)
}

// ---- the output: a workgroup per graph, a wave per path ------------------------------------------------------------------------
__global__ __launch_bounds__(PATHS_EMIT_THREADS) void paths_emit_kernel(PathsParams p) {
    if (*p.fits != PATHS_FITS_YES) return;
    const uint32_t g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = p.n_graphs;
    const uint32_t np = p.g_counts[(size_t)PATHS_COUNTS * g + PATHS_C_PATHS];
    const uint32_t P0 = p.out_off[g], E0 = p.out_off[(size_t)(n + 1) + g], B0 = p.out_off[2 * (size_t)(n + 1) + g];
    if (g == n - 1 && threadIdx.x == 0) p.hap_off[p.out_off[n]] = p.out_off[2 * (size_t)(n + 1) + n];
    if (!np) return;
    const Graph G = load_graph(p, g);
    const u64 nb = p.node_off[g];
    const Tree t{p.n_parent + nb, p.n_edge + nb, p.n_vertex + nb, p.n_len + nb, p.n_bytes + nb, p.n_score + nb, p.n_is_ref + nb};
    const uint32_t *const r_node = p.r_node + nb;
    uint32_t *const r_edge_off = p.q_node + nb;  // the queue is done with: where each path's edges start
    if (wave == 0) {
        uint32_t run_e = E0, run_b = B0;
        for (uint32_t base = 0; base < np; base += 64) {
            const uint32_t r = base + lane, node = r < np ? r_node[r] : 0;
            const uint32_t le = r < np ? t.len[node] : 0, lb = r < np ? t.bytes[node] : 0;
            const uint32_t ie = (uint32_t)wave_inclusive_scan(le), ib = (uint32_t)wave_inclusive_scan(lb);
            if (r < np) {
                p.path_score[P0 + r] = t.score[node], p.path_is_ref[P0 + r] = t.is_ref[node], p.path_n_edges[P0 + r] = le;
                p.hap_off[P0 + r] = run_b + ib - lb, r_edge_off[r] = run_e + ie - le;
            }
            run_e += __shfl(ie, 63), run_b += __shfl(ib, 63);
        }
    }
    __syncthreads();
    for (uint32_t r = wave; r < np; r += PATHS_EMIT_THREADS / 64) {
        uint32_t node = r_node[r];
        const uint32_t hb = p.hap_off[P0 + r], eo = r_edge_off[r];
        for (uint32_t step = 0; step <= G.nv; ++step) {  // Path::get_bases (path.rs:234-267), from the last vertex to the first
            const uint32_t v = t.vertex[node], vl = G.vlen(v), ln = t.len[node];
            const uint8_t *const from = p.bases + G.b0 + G.vbo[v];
            uint8_t *const to = p.hap_bases + hb + (t.bytes[node] - vl);
            for (uint32_t i = lane; i < vl; i += 64) to[i] = from[i];
            if (!ln) break;
            if (lane == 0) p.path_edges[eo + ln - 1] = t.edge[node];
            node = t.parent[node];
        }
    }
}

// ---- the duplicate marks: a wave per path, lengths first, then 256 bytes per pass ----------------------------------------------
__device__ bool bytes_equal(const uint8_t *a, const uint8_t *b, uint32_t len) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = 0; base < len; base += 256) {
        bool diff = false;
        for (uint32_t i = base + 4 * lane; i < base + 4 * lane + 4 && i < len; ++i) diff |= a[i] != b[i];
        if (__any(diff)) return false;
    }
    return true;
}
__global__ __launch_bounds__(PATHS_EMIT_THREADS) void paths_duplicates_kernel(PathsParams p) {
    if (*p.fits != PATHS_FITS_YES) return;
    const uint32_t lane = threadIdx.x & 63, n = p.n_graphs, total = p.out_off[n];
    const uint32_t path = blockIdx.x * (PATHS_EMIT_THREADS / 64) + (threadIdx.x >> 6);
    if (path >= total) return;
    uint32_t lo = 0, hi = n;  // the graph whose paths hold `path`: the last one that starts at or before it
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p.out_off[mid] <= path) lo = mid;
        else hi = mid;
    }
    const uint32_t g = lo, region = g % p.n_regions, k = g / p.n_regions;
    const uint32_t len = p.hap_off[path + 1] - p.hap_off[path];
    const uint8_t *const mine = p.hap_bases + p.hap_off[path];
    uint32_t answer = PATHS_NONE;
    const uint32_t r0 = p.region_ref_off[region], rl = p.region_ref_off[region + 1] - r0;
    if (rl == len && bytes_equal(mine, p.ref_bases + r0, len)) {
        answer = PATHS_EQUALS_REF;
    } else {
        for (uint32_t kk = 0; kk <= k && answer == PATHS_NONE; ++kk) {  // what find_best_path met before: k order, rank order
            const uint32_t gg = kk * p.n_regions + region, first = p.out_off[gg], last = kk == k ? path : p.out_off[gg + 1];
            for (uint32_t base = first; base < last && answer == PATHS_NONE; base += 64) {
                const uint32_t q = base + lane;
                u64 m = __ballot(q < last && p.hap_off[q + 1] - p.hap_off[q] == len);
                while (m) {
                    const uint32_t c = base + (uint32_t)__ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (bytes_equal(mine, p.hap_bases + p.hap_off[c], len)) {
                        answer = c;
                        break;
                    }
                }
            }
        }
    }
    if (lane == 0) p.path_first_equal[path] = answer;
}

}  // namespace

hipError_t launch_paths(const PathsParams &p, hipStream_t stream) {
    if (!p.n_graphs) return hipSuccess;
    hipLaunchKernelGGL(paths_search_kernel, dim3(p.n_graphs), dim3(PATHS_THREADS), 0, stream, p);
    hipLaunchKernelGGL(paths_offsets_kernel, dim3(1), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(paths_emit_kernel, dim3(p.n_graphs), dim3(PATHS_EMIT_THREADS), 0, stream, p);
    if (p.path_first_equal && p.capacity[0]) {
        const uint32_t waves = PATHS_EMIT_THREADS / 64;
        hipLaunchKernelGGL(paths_duplicates_kernel, dim3((p.capacity[0] + waves - 1) / waves), dim3(PATHS_EMIT_THREADS), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace phmm
