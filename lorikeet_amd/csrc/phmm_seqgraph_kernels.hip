// phmm_assembly_seqgraph (include/phmm.h): what the assembler does between the pruned read-threading graph and simplify_graph --
// to_sequence_graph (base_graph.rs:54-84), clean_non_ref_paths (base_graph.rs:716-768), the first zip_linear_chains
// (seq_graph.rs:189-369), remove_singleton_orphan_vertices (base_graph.rs:392-406) and
// remove_vertices_not_connected_to_ref_regardless_of_edge_direction (base_graph.rs:774-793).
//
// Three kernels on one stream.  seqgraph_kernel: one workgroup per graph, passes separated by workgroup barriers; integers,
// bytes and atomics; it leaves the graph's sizes and, in the workspace, where every output element goes.  seqgraph_offsets: one
// workgroup sums the sizes over the graphs and compares them with the capacities.  seqgraph_emit: one workgroup per graph
// writes the vertices, the bytes and the edges at the graph's offsets, if everything fits.
//
// The reference states each step serially; none of the results depends on that order except the numbering:
//   clean     the removed edges are a least fixed point: relaxed until a round changes nothing.  A vertex's list is pushed once
//             per removed edge that leaves it towards the swept end, and once more for the end itself
//   chains    a vertex continues its one predecessor's chain if that predecessor has out-degree 1, is another vertex and has the
//             same is_reference_node.  Pointer jumping (ping-pong, ceil(log2(vertices + 1)) + 1 rounds) gives the chain's first
//             vertex and the distance from it; a vertex whose last ancestor still continues a chain lies on a ring.  A chain is
//             merged if its first vertex is a zip start and it has two vertices or more.  Only a chain's first vertex can carry
//             k bytes, so a member's byte lies at (first's bytes + distance - 1): no segmented sum is needed
//   numbering a merged vertex takes the slot of its chain's first vertex.  Zip starts are listed in ascending index, so merged
//             vertices follow the unmerged ones in the order of their first vertices: two prefix sums over the vertices
//   edges     an edge inside a merged chain goes.  An edge that touches no merged chain keeps its place.  Every other edge is
//             re-created when the chain at its source (phase A of that merge: the last vertex's out-edges, newest first) or at
//             its target (phase B: the first vertex's in-edges, newest first) merges, twice if both do; it is numbered by
//             (time of its last creation, phase, re-created edges before originals, newest first), a 128-bit key that a bitonic
//             sort ranks.  The merge time of a chain is the index of its first vertex
// Every sweep ends after vertices + 1 rounds, the jumps after their logarithm, the sort after its passes.
#include "phmm_seqgraph_internal.hpp"

namespace phmm {
namespace {

enum { S_COUNT0, S_CLEAN, S_FAIL, S_ZIPPED, S_ZCOUNT, S_UNCONN, S_NT, S_SOURCE, S_SINK, S_ZSRC, S_WORDS };

struct Graph {
    uint32_t v0, nv, e0, ne, kk;
    const uint32_t *src, *dst;
    const uint8_t *is_ref;
    uint32_t *w;
    uint64_t stride;
    __device__ uint32_t *plane(int i) const { return w + (uint64_t)i * stride + v0; }
};

__device__ Graph graph_of(const SeqParams &p, uint32_t g) {
    Graph G;
    G.v0 = p.vertex_off[g];
    G.nv = p.vertex_off[g + 1] - G.v0;
    G.e0 = p.edge_off[g];
    G.ne = p.edge_off[g + 1] - G.e0;
    G.kk = p.k[g / p.n_regions];
    G.src = p.edge_src + G.e0;
    G.dst = p.edge_dst + G.e0;
    G.is_ref = p.edge_is_ref + G.e0;
    G.w = p.w;
    G.stride = p.v_total;
    return G;
}

__device__ int jump_rounds(uint32_t nv) { return (nv ? 32 - __clz(nv) : 0) + 1; }  // ceil(log2(vertices + 1)) + 1

// the exclusive prefix of x over the workgroup's threads, and the sum of all
__device__ uint32_t block_scan(uint32_t x, uint32_t *buf, uint32_t tid, uint32_t *total) {
    buf[tid] = x;
    __syncthreads();
    for (uint32_t off = 1; off < SEQ_THREADS; off <<= 1) {
        const uint32_t t = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += t;
        __syncthreads();
    }
    const uint32_t incl = buf[tid];
    *total = buf[SEQ_THREADS - 1];
    __syncthreads();
    return incl - x;
}

// the sort key of an edge that touches a merged chain: X / Y = the first vertex of the merged chain at its source / target
__device__ void edge_key(uint32_t e, uint32_t X, uint32_t Y, uint64_t *hi, uint64_t *lo) {
    constexpr uint64_t A = 0, B = 1;
    if (Y == SEQ_NONE) {
        *hi = (uint64_t)X << 2 | A << 1 | 1;
        *lo = ~(uint64_t)e;
    } else if (X == SEQ_NONE) {
        *hi = (uint64_t)Y << 2 | B << 1 | 1;
        *lo = ~(uint64_t)e;
    } else if (X <= Y) {  // created at X's merge (phase A), created again at Y's (phase B; the same merge if X == Y)
        *hi = (uint64_t)Y << 2 | B << 1;
        *lo = ~((uint64_t)X << 33 | A << 32 | (uint64_t)(~e));
    } else {
        *hi = (uint64_t)X << 2 | A << 1;
        *lo = ~((uint64_t)Y << 33 | B << 32 | (uint64_t)(~e));
    }
}

__device__ bool key_less(uint64_t ah, uint64_t al, uint64_t bh, uint64_t bl) { return ah < bh || (ah == bh && al < bl); }

__global__ __launch_bounds__(SEQ_THREADS) void seqgraph_kernel(SeqParams p) {
    const uint32_t g = blockIdx.x, tid = threadIdx.x, T = SEQ_THREADS;
    const Graph G = graph_of(p, g);
    const uint32_t nv = G.nv, ne = G.ne, kk = G.kk;
    const uint32_t *const src = G.src, *const dst = G.dst;
    const uint8_t *const is_ref = G.is_ref;
    const uint8_t *const v_absent = p.vertex_absent ? p.vertex_absent + G.v0 : nullptr, *const e_absent = p.edge_absent ? p.edge_absent + G.e0 : nullptr;
    uint32_t *const v_flags = G.plane(SEQ_V_FLAGS), *const v_in = G.plane(SEQ_V_IN), *const v_out = G.plane(SEQ_V_OUT), *const v_ref = G.plane(SEQ_V_REF),
                    *const v_blen = G.plane(SEQ_V_BLEN), *const v_mark = G.plane(SEQ_V_MARK), *const v_push = G.plane(SEQ_V_PUSH),
                    *const v_held = G.plane(SEQ_V_HELD), *const v_pred = G.plane(SEQ_V_PRED), *const v_link = G.plane(SEQ_V_LINK),
                    *const v_clen = G.plane(SEQ_V_CLEN), *const v_rep = G.plane(SEQ_V_REP), *const v_zin = G.plane(SEQ_V_ZIN),
                    *const v_zout = G.plane(SEQ_V_ZOUT), *const v_zref = G.plane(SEQ_V_ZREF), *const v_outidx = G.plane(SEQ_V_OUTIDX),
                    *const v_byteoff = G.plane(SEQ_V_BYTEOFF);
    uint8_t *const e_state = p.e_state + G.e0;
    uint32_t *const e_pos = p.e_pos + G.e0;
    uint64_t *const keys = p.keys + 2ull * p.key_off[g];
    uint32_t *const to_seq = p.vertex_to_seq + G.v0;
    uint32_t *const counts = p.g_counts + (uint64_t)SEQ_COUNTS * g;
    // a thread's contiguous runs of edges and of vertices, for the sweeps and the prefix sums
    const uint32_t per_e = ne / T + (ne % T != 0), per_v = nv / T + (nv % T != 0);
    const uint32_t elo = (uint64_t)tid * per_e < ne ? tid * per_e : ne, ehi = ne - elo < per_e ? ne : elo + per_e;
    const uint32_t vlo = (uint64_t)tid * per_v < nv ? tid * per_v : nv, vhi = nv - vlo < per_v ? nv : vlo + per_v;
    const uint32_t max_rounds = nv + 1;

    __shared__ uint32_t s[S_WORDS];
    __shared__ uint32_t scan[SEQ_THREADS];
    if (tid < S_WORDS) s[tid] = tid >= S_SOURCE ? SEQ_NONE : 0;
    __syncthreads();

    const auto leave = [&](uint32_t status) {  // a graph without an output graph
        for (uint32_t v = tid; v < nv; v += T) to_seq[v] = SEQ_NONE;
        if (tid < SEQ_COUNTS) counts[tid] = tid == SEQ_C_STATUS ? status : tid >= SEQ_C_SOURCE ? SEQ_NONE : 0;
    };
    if (p.graph_flags && (p.graph_flags[g] & 3u)) {  // PHMM_PRUNE_HAS_CYCLE | PHMM_PRUNE_NO_REF_ENDS: the caller drops it
        leave(SEQ_SKIPPED);
        return;
    }

    // ---- (1) the conversion: present elements, degrees, who carries k bytes (B:54-84) ------------------------------------------
    uint32_t n = 0;
    for (uint32_t v = tid; v < nv; v += T) {
        const bool absent = v_absent && v_absent[v];
        v_flags[v] = absent ? SEQ_F_GONE : 0;
        v_in[v] = v_out[v] = v_ref[v] = v_clen[v] = v_zin[v] = v_zout[v] = v_zref[v] = 0;
        v_pred[v] = SEQ_NONE;
        n += !absent;
    }
    if (n) atomicAdd(&s[S_COUNT0], n);
    for (uint32_t e = tid; e < ne; e += T) e_state[e] = e_absent && e_absent[e] ? SEQ_E_ABSENT : 0;
    __syncthreads();
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
    uint32_t count = s[S_COUNT0];
    for (uint32_t v = tid; v < nv; v += T) {
        if (v_flags[v] & SEQ_F_GONE) continue;
        v_blen[v] = v_in[v] ? 1 : kk;
        const uint32_t r = v_ref[v];
        if (!(r & 1) && ((r & 2) || count == 1)) atomicMin(&s[S_SOURCE], v);  // B:339-387, B:411-428
        if (!(r & 2) && ((r & 1) || count == 1)) atomicMin(&s[S_SINK], v);
    }
    __syncthreads();

    // ---- (2) clean_non_ref_paths (B:716-768) -------------------------------------------------------------------------------------
    if (s[S_SOURCE] != SEQ_NONE && s[S_SINK] != SEQ_NONE) {
        for (int half = 0; half < 2; ++half) {
            // in front of the source an edge goes if its target is reached, and its source is reached then; behind the sink the mirror
            const uint32_t *const from = half ? src : dst, *const to = half ? dst : src;
            const uint32_t end = half ? s[S_SINK] : s[S_SOURCE];
            for (uint32_t v = tid; v < nv; v += T) {
                v_mark[v] = v == end;
                v_push[v] = v == end;
                v_held[v] = 0;
            }
            __syncthreads();
            for (uint32_t e = tid; e < ne; e += T)
                if (!e_state[e] && !is_ref[e]) v_held[from[e]] = 1;
            __syncthreads();
            n = 0;
            for (uint32_t r = 0; r < max_rounds; ++r) {
                int changed = 0;
                for (uint32_t e = elo; e < ehi; ++e) {
                    if (e_state[e] || is_ref[e] || !v_mark[from[e]]) continue;
                    e_state[e] = SEQ_E_CLEANED;
                    atomicSub(&v_out[src[e]], 1u);
                    atomicSub(&v_in[dst[e]], 1u);
                    atomicAdd(&v_push[to[e]], 1u);
                    v_mark[to[e]] = 1;
                    changed = 1;
                    ++n;
                }
                if (!__syncthreads_or(changed)) break;
            }
            if (n) atomicAdd(&s[S_CLEAN], n);
            // the reference pops an edge twice where a list with a non-reference edge is pushed twice, and panics on the second
            n = 0;
            for (uint32_t v = tid; v < nv; v += T) n |= v_push[v] >= 2 && v_held[v];
            if (n) s[S_FAIL] = 1;
            __syncthreads();
            if (s[S_FAIL]) {
                leave(SEQ_REFERENCE_FAILS);
                return;
            }
        }
        if (count != 1) {  // B:766: an isolated vertex is no reference source unless it is the only vertex
            n = 0;
            for (uint32_t v = tid; v < nv; v += T)
                if (!(v_flags[v] & SEQ_F_GONE) && !v_in[v] && !v_out[v]) {
                    v_flags[v] = SEQ_F_GONE;
                    ++n;
                }
            if (n) atomicSub(&s[S_COUNT0], n);
        }
        __syncthreads();
    }

    // ---- (3) zip_linear_chains (S:189-369): starts, links, chains ---------------------------------------------------------------
    for (uint32_t e = tid; e < ne; e += T)
        if (!e_state[e] && v_in[dst[e]] == 1) v_pred[dst[e]] = src[e];
    __syncthreads();
    uint32_t *anc = G.plane(SEQ_V_ANC0), *dist = G.plane(SEQ_V_DIST0), *anc2 = G.plane(SEQ_V_ANC1), *dist2 = G.plane(SEQ_V_DIST1);
    for (uint32_t v = tid; v < nv; v += T) {
        uint32_t link = SEQ_NONE;
        if (!(v_flags[v] & SEQ_F_GONE)) {
            const uint32_t pr = v_pred[v];
            const bool one_in = v_in[v] == 1 && pr != SEQ_NONE;
            if (v_out[v] == 1 && (!one_in || v_out[pr] > 1)) v_flags[v] |= SEQ_F_START;     // S:227-238
            if (one_in && v_out[pr] == 1 && pr != v && !v_ref[pr] == !v_ref[v]) link = pr;   // S:257-284
        }
        v_link[v] = link;
        anc[v] = link == SEQ_NONE ? v : link;
        dist[v] = link != SEQ_NONE;
    }
    __syncthreads();
    for (int r = jump_rounds(nv); r > 0; --r) {
        for (uint32_t v = tid; v < nv; v += T) {
            const uint32_t a = anc[v], d = dist[v] + dist[a];
            anc2[v] = anc[a];
            dist2[v] = d < 0x7fffffffu ? d : 0x7fffffffu;  // (a ring's distances only grow)
        }
        __syncthreads();
        uint32_t *t = anc;
        anc = anc2;
        anc2 = t;
        t = dist;
        dist = dist2;
        dist2 = t;
    }
    for (uint32_t v = tid; v < nv; v += T) {
        if (v_flags[v] & SEQ_F_GONE) continue;
        const uint32_t a = anc[v];
        if (v_link[a] == SEQ_NONE && (v_flags[a] & SEQ_F_START)) atomicMax(&v_clen[a], dist[v] + 1);
    }
    __syncthreads();
    n = 0;
    uint32_t n_alive = 0;
    for (uint32_t v = tid; v < nv; v += T) {
        const uint32_t f = v_flags[v];
        v_rep[v] = v;
        v_mark[v] = 0;
        if (f & SEQ_F_GONE) continue;
        const uint32_t a = anc[v];
        if (v_link[a] == SEQ_NONE && (v_flags[a] & SEQ_F_START) && v_clen[a] >= 2) {
            v_rep[v] = a;
            v_flags[v] = f | SEQ_F_MERGED | (a == v ? SEQ_F_ALIVE : 0);
            n += a == v;
            n_alive += a == v;
        } else {
            v_flags[v] = f | SEQ_F_ALIVE;
            ++n_alive;
        }
    }
    if (n) atomicAdd(&s[S_ZIPPED], n);
    if (n_alive) atomicAdd(&s[S_ZCOUNT], n_alive);
    __syncthreads();
    // the zipped graph on the slots: an edge inside a merged chain goes with the chain's vertices
    for (uint32_t e = tid; e < ne; e += T) {
        if (e_state[e]) continue;
        const uint32_t a = src[e], b = dst[e];
        if ((v_flags[a] & v_flags[b] & SEQ_F_MERGED) && v_link[b] == a) {
            e_state[e] = SEQ_E_INTERIOR;
            continue;
        }
        atomicAdd(&v_zout[v_rep[a]], 1u);
        atomicAdd(&v_zin[v_rep[b]], 1u);
        if (is_ref[e]) {
            atomicOr(&v_zref[v_rep[a]], 2u);
            atomicOr(&v_zref[v_rep[b]], 1u);
        }
    }
    __syncthreads();

    // ---- (4) orphans (B:392-406), (5) what the reference source reaches, forwards or backwards (B:774-793) ---------------------
    uint32_t zcount = s[S_ZCOUNT];
    if (zcount != 1) {
        n = 0;
        for (uint32_t v = tid; v < nv; v += T)
            if ((v_flags[v] & SEQ_F_ALIVE) && !v_zin[v] && !v_zout[v]) {
                v_flags[v] &= ~SEQ_F_ALIVE;
                ++n;
            }
        if (n) atomicSub(&s[S_ZCOUNT], n);
    }
    __syncthreads();
    zcount = s[S_ZCOUNT];
    // (the lowest model index: unmerged vertices by their index, merged ones behind them by their first vertex)
    for (uint32_t v = tid; v < nv; v += T) {
        const uint32_t f = v_flags[v], r = v_zref[v];
        if ((f & SEQ_F_ALIVE) && !(r & 1) && ((r & 2) || zcount == 1)) atomicMin(&s[S_ZSRC], (f & SEQ_F_MERGED) ? 0x80000000u | v : v);
    }
    __syncthreads();
    if (s[S_ZSRC] != SEQ_NONE) {
        if (tid == 0) v_mark[s[S_ZSRC] & 0x7fffffffu] = 3;
        __syncthreads();
        for (uint32_t r = 0; r < max_rounds; ++r) {  // forwards: only bit 0 changes
            int changed = 0;
            for (uint32_t e = elo; e < ehi; ++e) {
                if (e_state[e]) continue;
                const uint32_t b = v_rep[dst[e]], m = v_mark[b];
                if ((v_mark[v_rep[src[e]]] & 1) && !(m & 1)) {
                    v_mark[b] = m | 1;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (uint32_t r = 0; r < max_rounds; ++r) {  // backwards: only bit 1 changes
            int changed = 0;
            for (uint32_t e = ehi; e-- > elo;) {
                if (e_state[e]) continue;
                const uint32_t a = v_rep[src[e]], m = v_mark[a];
                if ((v_mark[v_rep[dst[e]]] & 2) && !(m & 2)) {
                    v_mark[a] = m | 2;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
    }
    n = 0;
    for (uint32_t v = tid; v < nv; v += T)
        if ((v_flags[v] & SEQ_F_ALIVE) && !v_mark[v]) {
            v_flags[v] &= ~SEQ_F_ALIVE;
            ++n;
        }
    if (n) atomicAdd(&s[S_UNCONN], n);
    __syncthreads();

    // ---- the numbering: unmerged vertices in their order, then merged ones in the order of their first vertices ----------------
    uint32_t c_un = 0, b_un = 0, c_me = 0, b_me = 0;
    for (uint32_t v = vlo; v < vhi; ++v) {
        const uint32_t f = v_flags[v];
        if (!(f & SEQ_F_ALIVE)) continue;
        if (f & SEQ_F_MERGED) {
            ++c_me;
            b_me += v_blen[v] + v_clen[v] - 1;
        } else {
            ++c_un;
            b_un += v_blen[v];
        }
    }
    uint32_t n_un, nb_un, n_me, nb_me;
    uint32_t at_un = block_scan(c_un, scan, tid, &n_un), at_bun = block_scan(b_un, scan, tid, &nb_un);
    uint32_t at_me = n_un + block_scan(c_me, scan, tid, &n_me), at_bme = nb_un + block_scan(b_me, scan, tid, &nb_me);
    for (uint32_t v = vlo; v < vhi; ++v) {
        const uint32_t f = v_flags[v];
        if (!(f & SEQ_F_ALIVE)) continue;
        if (f & SEQ_F_MERGED) {
            v_outidx[v] = at_me++;
            v_byteoff[v] = at_bme;
            at_bme += v_blen[v] + v_clen[v] - 1;
        } else {
            v_outidx[v] = at_un++;
            v_byteoff[v] = at_bun;
            at_bun += v_blen[v];
        }
        v_zref[v] = 0;
    }
    __syncthreads();
    for (uint32_t v = tid; v < nv; v += T) {
        const uint32_t f = v_flags[v];
        to_seq[v] = !(f & SEQ_F_GONE) && (v_flags[v_rep[v]] & SEQ_F_ALIVE) ? v_outidx[v_rep[v]] : SEQ_NONE;
    }

    // ---- the edges: untouched ones keep their order, re-created ones follow by their keys --------------------------------------
    uint32_t c_keep = 0;
    for (uint32_t e = elo; e < ehi; ++e) {
        if (e_state[e]) continue;
        const uint32_t fa = v_flags[src[e]], fb = v_flags[dst[e]];
        if (!(v_flags[v_rep[src[e]]] & v_flags[v_rep[dst[e]]] & SEQ_F_ALIVE)) {
            e_state[e] = SEQ_E_DROPPED;
            continue;
        }
        if (is_ref[e]) {  // the reference bits of the graph that is left
            atomicOr(&v_zref[v_rep[src[e]]], 2u);
            atomicOr(&v_zref[v_rep[dst[e]]], 1u);
        }
        if ((fa | fb) & SEQ_F_MERGED) {
            const uint32_t i = atomicAdd(&s[S_NT], 1u);  // (any order: the sort follows)
            edge_key(e, (fa & SEQ_F_MERGED) ? v_rep[src[e]] : SEQ_NONE, (fb & SEQ_F_MERGED) ? v_rep[dst[e]] : SEQ_NONE, &keys[2ull * i], &keys[2ull * i + 1]);
        } else {
            ++c_keep;
        }
    }
    uint32_t n_keep;
    uint32_t at_keep = block_scan(c_keep, scan, tid, &n_keep);
    const uint32_t nt = s[S_NT];
    for (uint32_t e = elo; e < ehi; ++e)
        if (!e_state[e] && !((v_flags[src[e]] | v_flags[dst[e]]) & SEQ_F_MERGED)) e_pos[e] = at_keep++;
    uint32_t np2 = 1;
    while (np2 < nt) np2 <<= 1;  // (<= the graph's sort slots: nt <= edges)
    if (nt) {
        for (uint32_t i = nt + tid; i < np2; i += T) keys[2ull * i] = keys[2ull * i + 1] = ~0ull;
        __syncthreads();
        for (uint32_t k2 = 2; k2 <= np2; k2 <<= 1)
            for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                for (uint32_t i = tid; i < np2; i += T) {
                    const uint32_t l = i ^ j;
                    if (l <= i) continue;
                    const uint64_t ah = keys[2ull * i], al = keys[2ull * i + 1], bh = keys[2ull * l], bl = keys[2ull * l + 1];
                    if (key_less(bh, bl, ah, al) == !(i & k2)) {
                        keys[2ull * i] = bh;
                        keys[2ull * i + 1] = bl;
                        keys[2ull * l] = ah;
                        keys[2ull * l + 1] = al;
                    }
                }
                __syncthreads();
            }
        for (uint32_t e = tid; e < ne; e += T) {
            if (e_state[e]) continue;
            const uint32_t fa = v_flags[src[e]], fb = v_flags[dst[e]];
            if (!((fa | fb) & SEQ_F_MERGED)) continue;
            uint64_t hi, lo;
            edge_key(e, (fa & SEQ_F_MERGED) ? v_rep[src[e]] : SEQ_NONE, (fb & SEQ_F_MERGED) ? v_rep[dst[e]] : SEQ_NONE, &hi, &lo);
            uint32_t a = 0, b = nt;  // the keys differ: the first slot that is not below the edge's key holds it
            while (a < b) {
                const uint32_t m = a + (b - a) / 2;
                if (key_less(keys[2ull * m], keys[2ull * m + 1], hi, lo)) a = m + 1;
                else b = m;
            }
            e_pos[e] = n_keep + a;
        }
    }
    __syncthreads();
    // ---- the reference ends of the graph that is left ------------------------------------------------------------------------------
    if (tid == 0) s[S_SOURCE] = s[S_SINK] = SEQ_NONE;
    __syncthreads();
    const uint32_t n_left = n_un + n_me;
    for (uint32_t v = tid; v < nv; v += T) {
        const uint32_t f = v_flags[v], r = v_zref[v];
        if (!(f & SEQ_F_ALIVE)) continue;
        if (!(r & 1) && ((r & 2) || n_left == 1)) atomicMin(&s[S_SOURCE], v_outidx[v]);
        if (!(r & 2) && ((r & 1) || n_left == 1)) atomicMin(&s[S_SINK], v_outidx[v]);
    }
    __syncthreads();
    if (tid == 0) {
        counts[SEQ_C_STATUS] = SEQ_OK;
        counts[SEQ_C_VERTICES] = n_left;
        counts[SEQ_C_EDGES] = n_keep + nt;
        counts[SEQ_C_BASES] = nb_un + nb_me;
        counts[SEQ_C_ZIPPED] = s[S_ZIPPED];
        counts[SEQ_C_CLEAN] = s[S_CLEAN];
        counts[SEQ_C_UNCONNECTED] = s[S_UNCONN];
        counts[SEQ_C_SOURCE] = s[S_SOURCE];
        counts[SEQ_C_SINK] = s[S_SINK];
    }
}

// the graphs' offsets in the three output arrays, and whether the arrays hold everything
__global__ __launch_bounds__(SEQ_THREADS) void seqgraph_offsets(SeqParams p) {
    const uint32_t tid = threadIdx.x, T = SEQ_THREADS, ng = p.n_graphs;
    __shared__ uint32_t scan[SEQ_THREADS];
    const uint32_t per = ng / T + (ng % T != 0);
    const uint32_t lo = (uint64_t)tid * per < ng ? tid * per : ng, hi = ng - lo < per ? ng : lo + per;
    bool fits = true;
    for (int what = 0; what < 3; ++what) {
        uint32_t *const off = p.seq_off + (uint64_t)what * (ng + 1);
        uint32_t sum = 0, total;
        for (uint32_t g = lo; g < hi; ++g) sum += p.g_counts[(uint64_t)SEQ_COUNTS * g + SEQ_C_VERTICES + what];
        uint32_t at = block_scan(sum, scan, tid, &total);
        for (uint32_t g = lo; g < hi; ++g) {
            off[g] = at;
            at += p.g_counts[(uint64_t)SEQ_COUNTS * g + SEQ_C_VERTICES + what];
        }
        if (tid == 0) off[ng] = total;
        fits = fits && total <= p.capacity[what];
    }
    if (tid == 0) *p.fits = fits;
}

__global__ __launch_bounds__(SEQ_THREADS) void seqgraph_emit(SeqParams p) {
    const uint32_t g = blockIdx.x, tid = threadIdx.x, T = SEQ_THREADS;
    if (!*p.fits || p.g_counts[(uint64_t)SEQ_COUNTS * g + SEQ_C_STATUS] != SEQ_OK) return;
    const Graph G = graph_of(p, g);
    const uint32_t nv = G.nv, ne = G.ne, kk = G.kk;
    const uint32_t at_v = p.seq_off[g], at_e = p.seq_off[(uint64_t)p.n_graphs + 1 + g], at_b = p.seq_off[2ull * (p.n_graphs + 1) + g];
    const uint32_t *const v_flags = G.plane(SEQ_V_FLAGS), *const v_blen = G.plane(SEQ_V_BLEN), *const v_clen = G.plane(SEQ_V_CLEN),
                   *const v_rep = G.plane(SEQ_V_REP), *const v_outidx = G.plane(SEQ_V_OUTIDX), *const v_byteoff = G.plane(SEQ_V_BYTEOFF),
                   *const dist = G.plane(jump_rounds(nv) & 1 ? SEQ_V_DIST1 : SEQ_V_DIST0), *const v_base = p.vertex_base + G.v0;
    for (uint32_t v = tid; v < nv; v += T) {
        const uint32_t f = v_flags[v];
        if (f & SEQ_F_GONE) continue;
        const uint32_t h = v_rep[v];
        if (!(v_flags[h] & SEQ_F_ALIVE)) continue;
        uint8_t *const out = p.seq_bases + at_b + v_byteoff[h];
        if (h != v) {  // a chain's member behind its first vertex: its last byte
            out[v_blen[h] + dist[v] - 1] = p.bases[v_base[v] + kk - 1];
            continue;
        }
        const uint32_t i = at_v + v_outidx[v], len = v_blen[v];
        p.sv_base_off[i] = v_byteoff[v];
        p.sv_first[i] = v;
        p.sv_n_merged[i] = (f & SEQ_F_MERGED) ? v_clen[v] : 1;
        const uint8_t *const from = p.bases + v_base[v] + (kk - len);
        for (uint32_t j = 0; j < len; ++j) out[j] = from[j];
    }
    const uint8_t *const e_state = p.e_state + G.e0;
    for (uint32_t e = tid; e < ne; e += T) {
        if (e_state[e]) continue;
        const uint32_t j = at_e + p.e_pos[G.e0 + e];
        p.se_src[j] = v_outidx[v_rep[G.src[e]]];
        p.se_dst[j] = v_outidx[v_rep[G.dst[e]]];
        p.se_is_ref[j] = G.is_ref[e] != 0;
        p.se_mult[j] = p.edge_mult[G.e0 + e];
    }
}

}  // namespace

hipError_t launch_seqgraph(const SeqParams &p, hipStream_t stream) {
    if (!p.n_graphs) return hipSuccess;
    hipLaunchKernelGGL(seqgraph_kernel, dim3(p.n_graphs), dim3(SEQ_THREADS), 0, stream, p);
    hipLaunchKernelGGL(seqgraph_offsets, dim3(1), dim3(SEQ_THREADS), 0, stream, p);
    hipLaunchKernelGGL(seqgraph_emit, dim3(p.n_graphs), dim3(SEQ_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
