// phmm_assembly_graph (include/phmm.h): the raw read-threading graph as build_graph_if_necessary leaves it
// (read_threading_graph.rs:417-477) -- thread_sequence (:484-561), extend_chain_by_one (:700-769),
// increase_counts_in_matched_kmers (:641-687), MultiSampleEdge's heap (multi_sample_edge.rs) -- for many regions and several k
// at once, written without the threading order (DESIGN.md has the argument).  Integers and bytes only.  It runs behind the
// k-mer stage's kernels on the same stream and reads their prefix hashes, region tables and flag planes.
//   graph_order_kernel   a wave per (region, k): sample groups in order of their first read with a run, a read's threading rank
//   graph_vertex_kernel  a wave per (sequence, k), 64 positions a pass: a ballot gives every visited position its anchor, the
//                        nearest uniquely keyed position before it; its vertex is the anchor's k-mer slot (distance 0) or the
//                        bytes from the anchor on in the trie table; its edge (vertex before, vertex here) in the edge table;
//                        the lowest stamp into both
//   graph_count_kernel   a wave per (sequence, k): the creators per sequence, a vertex's two earliest in-edges
//   graph_scan_kernel    a wave per (region, k): the creators before each sequence in threading order, the graph's sizes
//  -- the host reads the sizes and lays the outputs out --
//   graph_index_kernel   a wave per (sequence, k): indices, the per-vertex and per-edge outputs a creator owns
//   graph_weight_kernel  a wave per (sequence, k): a count per traversal and (edge, group); the backward walk, a lane per
//                        sequence; the reference path and the vertex planes
//   graph_finish_kernel  a lane per edge: the multiplicity, and the heap's answer from the counts of the creator's group on
// Which position claims a slot is a race no output shows: what is read of a slot is who met in it (equal bytes, equal
// endpoints), the lowest stamp (atomicMin) and integer sums.
#include "phmm_graph_internal.hpp"

namespace phmm {

namespace {

using namespace asm_device;

__device__ inline const uint8_t *key_bases(const AsmParams &a, uint32_t key) {
    return key & ASM_READ_KEY ? a.read_bases + (key & ~ASM_READ_KEY) : a.ref_bases + key;
}

// what every per-sequence kernel knows of its wave's sequence
struct Walk {
    Seq s;
    uint32_t kk, k, w, r, g, o, rank, group;
    bool is_read, live;
    size_t plane;  // the sequence's first position in its k-major plane
};

__device__ inline Walk walk_of(const GraphParams &p) {
    const AsmParams &a = p.a;
    Walk x{};
    x.w = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6);
    x.live = x.w < a.n_regions + a.n_reads;
    if (!x.live) return x;
    x.kk = blockIdx.y;
    x.k = a.k[x.kk];
    x.is_read = x.w >= a.n_regions;
    x.r = x.w - a.n_regions;
    x.s = x.is_read ? read_seq(a, x.r) : ref_seq(a, x.w);
    x.g = x.s.region;
    x.o = x.kk * a.n_regions + x.g;
    x.live = ref_len(a, x.g) >= x.k;   // a REF_SHORT graph is empty
    x.rank = x.is_read ? p.read_rank[(size_t)x.kk * a.n_reads + x.r] : 0;
    x.group = x.is_read ? p.read_group[(size_t)x.kk * a.n_reads + x.r] : 0;
    x.plane = (size_t)x.kk * (x.is_read ? a.n_read_bases : a.n_ref_bases) + x.s.plane;
    return x;
}

__device__ inline unsigned long long stamp_of(const Walk &x, uint32_t pos) { return ((unsigned long long)x.rank << 32) | pos; }

// pending.entry(sample) (read_threading_graph.rs:328) is a LinkedHashMap: groups in order of the first read THAT YIELDS A
// SEQUENCE AT THIS K, reads in input order inside a group, the reference (A:984-994) in front of all
__global__ __launch_bounds__(64) void graph_order_kernel(GraphParams p) {
    __shared__ uint32_t first[GRAPH_MAX_SAMPLES], cnt[GRAPH_MAX_SAMPLES], gidx[GRAPH_MAX_SAMPLES], gbase[GRAPH_MAX_SAMPLES];
    const AsmParams &a = p.a;
    const uint32_t g = blockIdx.x, kk = blockIdx.y, lane = threadIdx.x, o = kk * a.n_regions + g;
    const uint32_t r0 = a.region_read_off[g], r1 = a.region_read_off[g + 1], S = p.region_n_samples[g];
    if (ref_len(a, g) < a.k[kk]) {
        if (lane == 0) p.n_yield[o] = 0, p.n_groups[o] = 1;
        return;
    }
    first[lane] = ASM_EMPTY;
    cnt[lane] = 0;
    __syncthreads();
    const uint32_t *runs = a.read_n_runs + (size_t)kk * a.n_reads;
    for (uint32_t base = r0; base < r1; base += 64) {
        const uint32_t r = base + lane;
        if (r < r1 && runs[r]) {
            atomicMin(&first[p.read_sample[r]], r);
            atomicAdd(&cnt[p.read_sample[r]], 1u);
        }
    }
    __syncthreads();
    const uint32_t f = first[lane];
    uint32_t before_groups = 0, before_reads = 0, all_reads = 0;
    for (uint32_t j = 0; j < S; ++j) {
        all_reads += cnt[j];
        if (first[j] < f) ++before_groups, before_reads += cnt[j];
    }
    gidx[lane] = before_groups + 1;
    gbase[lane] = before_reads + 1;
    const unsigned long long groups = __ballot(f != ASM_EMPTY);
    if (lane == 0) p.n_yield[o] = all_reads, p.n_groups[o] = 1 + (uint32_t)__popcll(groups);
    __syncthreads();
    uint32_t seen = 0;   // lane j: the reads of sample j so far
    for (uint32_t base = r0; base < r1; base += 64) {
        const uint32_t r = base + lane;
        const bool y = r < r1 && runs[r];
        const uint32_t s = y ? p.read_sample[r] : GRAPH_MAX_SAMPLES;
        uint32_t within = 0;
        for (uint32_t j = 0; j < S; ++j) {
            const unsigned long long m = __ballot(s == j);
            const uint32_t sj = __shfl(seen, j);
            if (s == j) within = sj + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            if (lane == j) seen += (uint32_t)__popcll(m);
        }
        if (y) {
            const uint32_t rank = gbase[s] + within;
            p.read_rank[(size_t)kk * a.n_reads + r] = rank;
            p.read_group[(size_t)kk * a.n_reads + r] = gidx[s];
            p.order[(size_t)kk * a.n_reads + r0 + rank - 1] = r;
        }
    }
}

// get_or_create_kmer_vertex (:597-605), extend_chain_by_one (:700-769), get_kmer_vertex (:613-618), track_kmer (:635-639):
// a k-mer that is not non-unique and not the reference source (away from a threading start) has the one vertex the map
// holds; every other visited position has the vertex keyed by (the vertex before it, its last base) -- the bytes from the
// nearest uniquely keyed position before it, its anchor, up to its own last base
__global__ __launch_bounds__(ASM_THREADS) void graph_vertex_kernel(GraphParams p) {
    const AsmParams &a = p.a;
    const Walk x = walk_of(p);
    if (!x.live) return;
    const uint32_t lane = threadIdx.x & 63, k = x.k;
    const uint8_t *fl = (x.is_read ? a.read_flags : a.ref_flags) + x.plane;
    const uint32_t *slot_of = (x.is_read ? a.read_slot : a.ref_slot) + x.plane;
    uint32_t *handle = (x.is_read ? p.read_handle : p.ref_handle) + x.plane, *edge = (x.is_read ? p.read_edge : p.ref_edge) + x.plane;
    // ref_source (:529-533) exists once the reference is threaded, that is, has more than k bases (:492)
    const uint32_t src_slot = ref_len(a, x.g) > k ? a.ref_slot[(size_t)x.kk * a.n_ref_bases + a.region_ref_off[x.g]] : ASM_EMPTY;
    const uint32_t t0 = a.region_table_off[x.g], rcap = a.region_table_off[x.g + 1] - t0, tb = x.kk * a.n_slots + t0;
    const uint32_t nh = a.n_k * a.n_slots;
    uint32_t carry_anchor = 0, carry_handle = ASM_EMPTY;
    for (uint32_t base = 0; base < x.s.len; base += 64) {
        const uint32_t pos = base + lane;
        const uint32_t f = pos < x.s.len ? fl[pos] : 0;
        const bool visited = f & ASM_THREADED, start = f & ASM_THREAD_START;
        const uint32_t slot = visited ? slot_of[pos] : ASM_EMPTY;
        const bool keyed = visited && (start || (!(f & ASM_NON_UNIQUE) && slot != src_slot));
        const unsigned long long am = __ballot(keyed), mine = am & (lane == 63 ? ~0ull : (2ull << lane) - 1);
        const uint32_t anchor = mine ? base + 63 - (uint32_t)__clzll((long long)mine) : carry_anchor;
        uint32_t h = ASM_EMPTY;
        const unsigned long long stamp = stamp_of(x, pos);
        if (visited) {
            const uint32_t d = pos - anchor;
            if (d == 0) {
                h = slot;
            } else {
                uint64_t pw = 1, b = ASM_HASH_BASE;
                for (uint32_t e = d + k; e; e >>= 1, b *= b)
                    if (e & 1) pw *= b;
                const uint64_t fp = mix64(x.s.hash[pos + k] - x.s.hash[anchor] * pw) & a.fp_mask;
                const uint32_t tag = (uint32_t)(fp ^ (fp >> 18) ^ (fp >> 36)) & 0x3ffffu;
                const uint32_t key = (x.is_read ? ASM_READ_KEY : 0u) | (x.s.plane + pos);
                const unsigned long long want = ((unsigned long long)tag << 46) | ((unsigned long long)d << 32) | key;
                uint32_t t = home_slot(fp, rcap);
                for (;; t = t + 1 == rcap ? 0 : t + 1) {
                    const unsigned long long prev = atomicCAS(&p.trie_claim[tb + t], GRAPH_NONE, want);
                    if (prev == GRAPH_NONE) break;
                    if ((prev >> 32) != (want >> 32)) continue;
                    if (same_bytes(key_bases(a, (uint32_t)prev) - d, x.s.bases + anchor, d + k)) break;
                }
                h = nh + tb + t;
            }
            atomicMin(&p.v_stamp[h], stamp);
            handle[pos] = h;
        }
        uint32_t before = __shfl_up(h, 1);
        if (lane == 0) before = carry_handle;
        if (visited && !start) {   // :761-765, or the edge found at :715-747: one edge per (source, target)
            const unsigned long long ekey = ((unsigned long long)before << 32) | h;
            uint32_t t = home_slot(mix64(ekey), rcap);
            for (;; t = t + 1 == rcap ? 0 : t + 1) {
                const unsigned long long prev = atomicCAS(&p.e_key[tb + t], GRAPH_NONE, ekey);
                if (prev == GRAPH_NONE || prev == ekey) break;
            }
            atomicMin(&p.e_stamp[tb + t], stamp);
            edge[pos] = tb + t;
        }
        carry_handle = __shfl(h, 63);
        if (am) carry_anchor = base + 63 - (uint32_t)__clzll((long long)am);
    }
}

// the occurrence with a slot's lowest stamp is its creator: petgraph numbers vertices and edges in that order
struct Creators {
    uint32_t h, e;
    bool vertex, edge;
};

__device__ inline Creators creators_at(const GraphParams &p, const Walk &x, uint32_t pos) {
    Creators c{ASM_EMPTY, ASM_EMPTY, false, false};
    if (pos >= x.s.len) return c;
    c.h = ((x.is_read ? p.read_handle : p.ref_handle) + x.plane)[pos];
    if (c.h == ASM_EMPTY) return c;
    const unsigned long long stamp = stamp_of(x, pos);
    c.vertex = p.v_stamp[c.h] == stamp;
    c.e = ((x.is_read ? p.read_edge : p.ref_edge) + x.plane)[pos];
    c.edge = c.e != ASM_EMPTY && p.e_stamp[c.e] == stamp;
    return c;
}

__global__ __launch_bounds__(ASM_THREADS) void graph_count_kernel(GraphParams p) {
    const Walk x = walk_of(p);
    if (!x.live) return;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t nv = 0, ne = 0;
    for (uint32_t base = 0; base < x.s.len; base += 64) {
        const uint32_t pos = base + lane;
        const Creators c = creators_at(p, x, pos);
        if (c.edge) {   // the two lowest of a set, in any order of arrival: what the lowest displaces, or what fails to displace it
            const unsigned long long stamp = stamp_of(x, pos), old = atomicMin(&p.v_in1[c.h], stamp);
            atomicMin(&p.v_in2[c.h], old > stamp ? old : stamp);
        }
        nv += (uint32_t)__popcll(__ballot(c.vertex));
        ne += (uint32_t)__popcll(__ballot(c.edge));
    }
    if (lane == 0) {
        const size_t i = (size_t)x.kk * (p.a.n_regions + p.a.n_reads) + x.w;
        p.seq_n_vertices[i] = nv;
        p.seq_n_edges[i] = ne;
    }
}

__global__ __launch_bounds__(64) void graph_scan_kernel(GraphParams p) {
    const AsmParams &a = p.a;
    const uint32_t g = blockIdx.x, kk = blockIdx.y, lane = threadIdx.x, o = kk * a.n_regions + g;
    const uint32_t n = 1 + p.n_yield[o], r0 = a.region_read_off[g], n_seq = a.n_regions + a.n_reads;
    uint32_t tv = 0, te = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        const bool in = i < n;
        const size_t at = (size_t)kk * n_seq + (!in || i == 0 ? g : a.n_regions + p.order[(size_t)kk * a.n_reads + r0 + i - 1]);
        const uint32_t cv = in ? p.seq_n_vertices[at] : 0, ce = in ? p.seq_n_edges[at] : 0;
        uint32_t sv = cv, se = ce;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t uv = __shfl_up(sv, d), ue = __shfl_up(se, d);
            if (lane >= d) sv += uv, se += ue;
        }
        if (in) {
            p.seq_vertex_base[at] = tv + sv - cv;
            p.seq_edge_base[at] = te + se - ce;
        }
        tv += __shfl(sv, 63);
        te += __shfl(se, 63);
    }
    if (lane == 0) {
        const uint32_t len = ref_len(a, g), k = a.k[kk];
        p.n_vertices[o] = tv;
        p.n_edges[o] = te;
        p.n_ref_path[o] = len > k ? len - k + 1 : 0;   // :492 returns in front of :525-528 for a reference of k bases
    }
}

__global__ __launch_bounds__(ASM_THREADS) void graph_index_kernel(GraphParams p) {
    const AsmParams &a = p.a;
    const Walk x = walk_of(p);
    if (!x.live) return;
    const uint32_t lane = threadIdx.x & 63, nh = a.n_k * a.n_slots;
    const uint32_t vo = p.vertex_off[x.o], eo = p.edge_off[x.o];
    const size_t at = (size_t)x.kk * (a.n_regions + a.n_reads) + x.w;
    uint32_t vb = p.seq_vertex_base[at], eb = p.seq_edge_base[at];
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t base = 0; base < x.s.len; base += 64) {
        const uint32_t pos = base + lane;
        const Creators c = creators_at(p, x, pos);
        const unsigned long long vm = __ballot(c.vertex), em = __ballot(c.edge);
        if (c.vertex) {
            const uint32_t i = vb + (uint32_t)__popcll(vm & below);
            p.v_index[c.h] = i;
            p.vertex_seq[vo + i] = x.is_read ? 1 + x.r - a.region_read_off[x.g] : 0;
            p.vertex_pos[vo + i] = pos;
            // kmer_to_vertex_map holds the uniquely keyed vertices (:635-639); the reference's first vertex is ref_source
            p.vertex_flags[vo + i] = (uint8_t)((c.h < nh && !(a.slot_bits[c.h] & ASM_NON_UNIQUE) ? GRAPH_VERTEX_TRACKED : 0) |
                                               (!x.is_read && pos == 0 ? GRAPH_VERTEX_REF_SOURCE : 0));
        }
        if (c.edge) {
            const uint32_t i = eb + (uint32_t)__popcll(em & below);
            p.e_index[c.e] = i;
            p.edge_is_ref[eo + i] = !x.is_read;
            p.edge_group[eo + i] = x.group;
            if (p.v_in1[c.h] == stamp_of(x, pos)) p.v_inedge[c.h] = c.e;
        }
        vb += (uint32_t)__popcll(vm);
        eb += (uint32_t)__popcll(em);
    }
}

__global__ __launch_bounds__(ASM_THREADS) void graph_weight_kernel(GraphParams p) {
    const AsmParams &a = p.a;
    const Walk x = walk_of(p);
    if (!x.live) return;
    const uint32_t lane = threadIdx.x & 63, nh = a.n_k * a.n_slots, k = x.k;
    const uint32_t eo = p.edge_off[x.o], width = p.count_width[x.o];
    uint32_t *counts = p.counts + p.count_off[x.o];
    const uint8_t *fl = (x.is_read ? a.read_flags : a.ref_flags) + x.plane;
    uint32_t *plane = p.want_planes ? (x.is_read ? p.read_vertex : p.ref_vertex) + x.plane : nullptr;
    for (uint32_t base = 0; base < x.s.len; base += 64) {
        const uint32_t pos = base + lane;
        const Creators c = creators_at(p, x, pos);
        if (c.h == ASM_EMPTY) continue;
        const uint32_t vi = p.v_index[c.h];
        if (plane) plane[pos] = vi;
        if (!x.is_read) p.ref_path[p.ref_path_off[x.o] + pos] = vi;   // :528, :546-548
        if (c.e != ASM_EMPTY) {
            const uint32_t ei = p.e_index[c.e];
            atomicAdd(&counts[(size_t)ei * width + x.group], 1u);      // the creation's count (:764) or inc_multiplicity (:745)
            if (c.edge) {
                p.edge_src[eo + ei] = p.v_index[(uint32_t)(p.e_key[c.e] >> 32)];
                p.edge_dst[eo + ei] = vi;
            }
        }
        if (!(fl[pos] & ASM_THREAD_START) || k < 2) continue;   // checked_sub(2) (:505): no walk for k = 1
        // increase_counts_in_matched_kmers (:641-687) without increase_counts_through_branches: a chain of single in-edges.
        // An edge existed when this sequence began if its creator's stamp is lower than the start's; original_kmer is the
        // WHOLE sequence (:504), so the offset counts from the sequence's first base whatever the start position
        const unsigned long long began = stamp_of(x, pos);
        uint32_t v = c.h;
        for (int off = (int)k - 2; off >= 0; --off) {
            if (!(p.v_in1[v] < began) || p.v_in2[v] < began) break;   // in_degree_of(vertex) == 1 (:670)
            const uint32_t e = p.v_inedge[v], src = (uint32_t)(p.e_key[e] >> 32);
            const uint32_t key = src < nh ? a.slot_rep[src] : (uint32_t)p.trie_claim[src - nh];
            if (key_bases(a, key)[k - 1] != x.s.bases[off]) break;    // get_suffix (:660-668)
            atomicAdd(&counts[(size_t)p.e_index[e] * width + x.group], 1u);
            v = src;
        }
    }
}

// multi_sample_edge.rs: the heap starts with the creation's count, takes the running count at every flush from the creator's
// group on (read_threading_graph.rs:454-456 flushes every edge that exists), drops its lowest once it holds capacity + 1, and
// get_pruning_multiplicity peeks the lowest
__global__ __launch_bounds__(ASM_THREADS) void graph_finish_kernel(GraphParams p) {
    const uint32_t o = blockIdx.x, i = blockIdx.y * ASM_THREADS + threadIdx.x;
    const uint32_t eo = p.edge_off[o];
    if (i >= p.edge_off[o + 1] - eo) return;
    const uint32_t width = p.count_width[o], n_groups = p.n_groups[o], cap = p.num_pruning_samples;
    const uint32_t *row = p.counts + p.count_off[o] + (size_t)i * width;
    uint32_t top[GRAPH_MAX_PRUNING_SAMPLES], held = 0, total = 0;
    const auto push = [&](uint32_t v) {
        for (uint32_t j = 0; j < held; ++j)
            if (v > top[j]) {
                const uint32_t t = top[j];
                top[j] = v;
                v = t;
            }
        if (held < cap) top[held++] = v;
    };
    push(1);
    for (uint32_t g = p.edge_group[eo + i]; g < n_groups; ++g) {
        total += row[g];
        push(row[g]);
    }
    p.edge_multiplicity[eo + i] = total;
    p.edge_pruning_multiplicity[eo + i] = top[held - 1];
}

}  // namespace

hipError_t launch_graph_build(const GraphParams &p, hipStream_t stream) {
    const AsmParams &a = p.a;
    hipError_t e = launch_assembly_kmers(a, stream);
    if (e != hipSuccess) return e;
    const size_t nk = a.n_k, n_ref = nk * a.n_ref_bases, n_read = nk * a.n_read_bases, n_slots = nk * a.n_slots;
    const size_t n_seq = nk * ((size_t)a.n_regions + a.n_reads);
    const auto fill = [&](void *dst, int v, size_t bytes) { return bytes ? hipMemsetAsync(dst, v, bytes, stream) : hipSuccess; };
    if ((e = fill(p.read_rank, 0, 4 * nk * a.n_reads)) != hipSuccess || (e = fill(p.read_group, 0, 4 * nk * a.n_reads)) != hipSuccess ||
        (e = fill(p.ref_handle, 0xff, 4 * n_ref)) != hipSuccess || (e = fill(p.read_handle, 0xff, 4 * n_read)) != hipSuccess ||
        (e = fill(p.ref_edge, 0xff, 4 * n_ref)) != hipSuccess || (e = fill(p.read_edge, 0xff, 4 * n_read)) != hipSuccess ||
        (e = fill(p.trie_claim, 0xff, 8 * n_slots)) != hipSuccess || (e = fill(p.v_stamp, 0xff, 16 * n_slots)) != hipSuccess ||
        (e = fill(p.v_in1, 0xff, 16 * n_slots)) != hipSuccess || (e = fill(p.v_in2, 0xff, 16 * n_slots)) != hipSuccess ||
        (e = fill(p.e_key, 0xff, 8 * n_slots)) != hipSuccess || (e = fill(p.e_stamp, 0xff, 8 * n_slots)) != hipSuccess ||
        (e = fill(p.seq_n_vertices, 0, 4 * n_seq)) != hipSuccess || (e = fill(p.seq_n_edges, 0, 4 * n_seq)) != hipSuccess)
        return e;
    const uint32_t waves = ASM_THREADS / 64;
    const dim3 graphs(a.n_regions, a.n_k), seqs((a.n_regions + a.n_reads + waves - 1) / waves, a.n_k);
    hipLaunchKernelGGL(graph_order_kernel, graphs, dim3(64), 0, stream, p);
    hipLaunchKernelGGL(graph_vertex_kernel, seqs, dim3(ASM_THREADS), 0, stream, p);
    hipLaunchKernelGGL(graph_count_kernel, seqs, dim3(ASM_THREADS), 0, stream, p);
    hipLaunchKernelGGL(graph_scan_kernel, graphs, dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_graph_fill(const GraphParams &p, hipStream_t stream) {
    const AsmParams &a = p.a;
    hipError_t e;
    const auto fill = [&](void *dst, int v, size_t bytes) { return bytes ? hipMemsetAsync(dst, v, bytes, stream) : hipSuccess; };
    if ((e = fill(p.counts, 0, 4 * (size_t)p.n_counts)) != hipSuccess) return e;
    if (p.want_planes && ((e = fill(p.ref_vertex, 0xff, 4 * (size_t)a.n_k * a.n_ref_bases)) != hipSuccess ||
                         (e = fill(p.read_vertex, 0xff, 4 * (size_t)a.n_k * a.n_read_bases)) != hipSuccess))
        return e;
    const uint32_t waves = ASM_THREADS / 64;
    const dim3 seqs((a.n_regions + a.n_reads + waves - 1) / waves, a.n_k);
    hipLaunchKernelGGL(graph_index_kernel, seqs, dim3(ASM_THREADS), 0, stream, p);
    hipLaunchKernelGGL(graph_weight_kernel, seqs, dim3(ASM_THREADS), 0, stream, p);
    if (p.max_edges)
        hipLaunchKernelGGL(graph_finish_kernel, dim3(a.n_k * a.n_regions, (p.max_edges + ASM_THREADS - 1) / ASM_THREADS), dim3(ASM_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
