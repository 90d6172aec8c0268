// The plain single-threaded host loop tools/assembly_seqgraph_bench.py times beside phmm_assembly_seqgraph, for scale: the same
// arrays in, the same arrays out (the bench compares them one by one).  It walks each graph the way the reference does -- a
// StableGraph's edge lists newest first, the heaps of clean_non_ref_paths, the chain walk of zip_linear_chains -- and shares no
// code with the library.  Build: make -C lorikeet_amd/csrc (tools/libassembly_seqgraph_host.so).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <queue>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xffffffffu;

struct SeqGraph {  // indices stay when an element goes; a new element takes a fresh index
    std::vector<char> node;
    std::vector<std::vector<uint8_t>> seq;
    std::vector<uint32_t> first, n_merged;
    std::vector<uint32_t> src, dst, mult;
    std::vector<uint8_t> is_ref, edge;
    std::vector<std::vector<uint32_t>> out, in;  // oldest first: walked backwards
    uint32_t count = 0;
    uint32_t add_node(std::vector<uint8_t> s, uint32_t f, uint32_t n) {
        node.push_back(1);
        seq.push_back(std::move(s));
        first.push_back(f);
        n_merged.push_back(n);
        out.emplace_back();
        in.emplace_back();
        ++count;
        return (uint32_t)node.size() - 1;
    }
    void add_edge(uint32_t a, uint32_t b, uint8_t r, uint32_t m) {
        src.push_back(a);
        dst.push_back(b);
        is_ref.push_back(r);
        mult.push_back(m);
        edge.push_back(1);
        out[a].push_back((uint32_t)src.size() - 1);
        in[b].push_back((uint32_t)src.size() - 1);
    }
    void remove_edge(uint32_t e) {
        auto &o = out[src[e]], &i = in[dst[e]];
        o.erase(std::find(o.begin(), o.end(), e));
        i.erase(std::find(i.begin(), i.end(), e));
        edge[e] = 0;
    }
    void remove_node(uint32_t v) {
        while (!out[v].empty()) remove_edge(out[v].back());
        while (!in[v].empty()) remove_edge(in[v].back());
        node[v] = 0;
        --count;
    }
    bool any_ref(const std::vector<uint32_t> &es) const {
        for (uint32_t e : es)
            if (is_ref[e]) return true;
        return false;
    }
    bool is_ref_source(uint32_t v) const { return !any_ref(in[v]) && (any_ref(out[v]) || count == 1); }
    bool is_ref_sink(uint32_t v) const { return !any_ref(out[v]) && (any_ref(in[v]) || count == 1); }
    bool is_reference_node(uint32_t v) const { return any_ref(in[v]) || any_ref(out[v]) || count == 1; }
    uint32_t find(bool sink) const {
        for (uint32_t v = 0; v < node.size(); ++v)
            if (node[v] && (sink ? is_ref_sink(v) : is_ref_source(v))) return v;
        return NONE;
    }
    void remove_orphans() {
        std::vector<uint32_t> gone;
        for (uint32_t v = 0; v < node.size(); ++v)
            if (node[v] && in[v].empty() && out[v].empty() && !is_ref_source(v)) gone.push_back(v);
        for (uint32_t v : gone) remove_node(v);
    }
};

struct Result {
    std::vector<uint32_t> counts, v_off{0}, e_off{0}, b_off{0}, base_off, first, n_merged, e_src, e_dst, e_mult, to_seq;
    std::vector<uint8_t> e_ref, bases;
} R;

// false: the reference fails
bool clean(SeqGraph &g, uint32_t &removed) {
    if (g.find(false) == NONE || g.find(true) == NONE) return true;
    for (int half = 0; half < 2; ++half) {
        const uint32_t end = g.find(half);
        if (end == NONE) return false;
        std::vector<uint32_t> pushes(g.node.size(), 0);
        std::vector<char> held(g.node.size(), 0);
        for (uint32_t e = 0; e < g.edge.size(); ++e)
            if (g.edge[e] && !g.is_ref[e]) held[half ? g.src[e] : g.dst[e]] = 1;
        std::priority_queue<uint32_t> heap;
        const auto push = [&](uint32_t v) {
            ++pushes[v];
            for (uint32_t e : half ? g.out[v] : g.in[v]) heap.push(e);
        };
        push(end);
        while (!heap.empty()) {
            const uint32_t e = heap.top();
            heap.pop();
            if (!g.edge[e] || g.is_ref[e]) continue;
            push(half ? g.dst[e] : g.src[e]);
            g.remove_edge(e);
            ++removed;
        }
        for (uint32_t v = 0; v < pushes.size(); ++v)
            if (pushes[v] >= 2 && held[v]) return false;  // the order-free contract of the header
    }
    g.remove_orphans();
    return true;
}

uint32_t zip(SeqGraph &g) {
    std::vector<uint32_t> starts;
    for (uint32_t v = 0; v < g.node.size(); ++v)
        if (g.node[v] && g.out[v].size() == 1 && (g.in[v].size() != 1 || g.out[g.src[g.in[v][0]]].size() > 1)) starts.push_back(v);
    uint32_t merged = 0;
    std::vector<uint32_t> chain;
    for (uint32_t s : starts) {
        chain.assign(1, s);
        uint32_t last = s;
        bool last_ref = g.is_reference_node(s);
        while (g.out[last].size() == 1) {
            const uint32_t t = g.dst[g.out[last][0]];
            if (g.in[t].size() != 1 || t == last) break;
            const bool t_ref = g.is_reference_node(t);
            if (t_ref != last_ref) break;
            chain.push_back(t);
            last = t;
            last_ref = t_ref;
        }
        if (chain.size() < 2) continue;
        std::vector<uint8_t> bytes;
        for (uint32_t v : chain) bytes.insert(bytes.end(), g.seq[v].begin(), g.seq[v].end());
        const uint32_t n = g.add_node(std::move(bytes), g.first[s], (uint32_t)chain.size());
        const std::vector<uint32_t> outs(g.out[last].rbegin(), g.out[last].rend());
        for (uint32_t e : outs) g.add_edge(n, g.dst[e], g.is_ref[e], g.mult[e]);
        const std::vector<uint32_t> ins(g.in[s].rbegin(), g.in[s].rend());
        for (uint32_t e : ins) g.add_edge(g.src[e], n, g.is_ref[e], g.mult[e]);
        for (uint32_t v : chain) g.remove_node(v);
        ++merged;
    }
    return merged;
}

uint32_t connect(SeqGraph &g) {
    std::vector<char> keep(g.node.size(), 0);
    const uint32_t s = g.find(false);
    if (s != NONE)
        for (int dir = 0; dir < 2; ++dir) {
            std::vector<uint32_t> stack{s};
            std::vector<char> seen(g.node.size(), 0);
            while (!stack.empty()) {
                const uint32_t v = stack.back();
                stack.pop_back();
                if (seen[v]) continue;
                seen[v] = keep[v] = 1;
                for (uint32_t e : dir ? g.out[v] : g.in[v]) stack.push_back(dir ? g.dst[e] : g.src[e]);
            }
        }
    uint32_t gone = 0;
    for (uint32_t v = 0; v < g.node.size(); ++v)
        if (g.node[v] && !keep[v]) {
            g.remove_node(v);
            ++gone;
        }
    return gone;
}

}  // namespace

// Computes every graph and keeps the result; sizes[3] = sequence vertices, edges, bytes.  The arrays are phmm_assembly_seqgraph's.
extern "C" void assembly_seqgraph_host(uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases, const uint32_t *region_read_off,
                                       const uint32_t *read_off, const uint8_t *read_bases, uint32_t n_k, const uint32_t *k, const uint32_t *vertex_off,
                                       const uint32_t *edge_off, const uint32_t *vertex_seq, const uint32_t *vertex_pos, const uint32_t *edge_src,
                                       const uint32_t *edge_dst, const uint8_t *edge_is_ref, const uint32_t *edge_multiplicity, const uint32_t *new_vertex_off,
                                       const uint8_t *new_vertex_kmer, const uint8_t *vertex_absent, const uint8_t *edge_absent, const uint32_t *graph_flags,
                                       uint32_t *sizes) {
    R = Result();
    const uint32_t n_graphs = n_k * n_regions;
    uint32_t k_max = 0;
    for (uint32_t i = 0; i < n_k; ++i) k_max = std::max(k_max, k[i]);
    R.to_seq.assign(vertex_off[n_graphs], NONE);
    for (uint32_t gi = 0; gi < n_graphs; ++gi) {
        const uint32_t v0 = vertex_off[gi], nv = vertex_off[gi + 1] - v0, e0 = edge_off[gi], ne = edge_off[gi + 1] - e0, reg = gi % n_regions, kk = k[gi / n_regions];
        uint32_t c[9] = {0, 0, 0, 0, 0, 0, 0, NONE, NONE};
        const auto close = [&] {
            R.counts.insert(R.counts.end(), c, c + 9);
            R.v_off.push_back((uint32_t)R.first.size());
            R.e_off.push_back((uint32_t)R.e_src.size());
            R.b_off.push_back((uint32_t)R.bases.size());
        };
        if (graph_flags && (graph_flags[gi] & 3)) {
            c[0] = 1;
            close();
            continue;
        }
        const uint32_t n_new = new_vertex_off ? new_vertex_off[gi + 1] - new_vertex_off[gi] : 0, n_raw = nv - n_new, raw0 = v0 - (new_vertex_off ? new_vertex_off[gi] : 0);
        SeqGraph g;
        std::vector<char> has_in(nv, 0);
        for (uint32_t e = 0; e < ne; ++e)
            if (!(edge_absent && edge_absent[e0 + e])) has_in[edge_dst[e0 + e]] = 1;
        std::vector<uint32_t> map(nv, NONE);
        for (uint32_t v = 0; v < nv; ++v) {
            if (vertex_absent && vertex_absent[v0 + v]) continue;
            const uint8_t *km;
            if (v >= n_raw) {
                km = new_vertex_kmer + (size_t)(new_vertex_off[gi] + (v - n_raw)) * k_max;
            } else {
                const uint32_t sq = vertex_seq[raw0 + v];
                km = (sq ? read_bases + read_off[region_read_off[reg] + sq - 1] : ref_bases + region_ref_off[reg]) + vertex_pos[raw0 + v];
            }
            map[v] = g.add_node(has_in[v] ? std::vector<uint8_t>(km + kk - 1, km + kk) : std::vector<uint8_t>(km, km + kk), v, 1);
        }
        for (uint32_t e = 0; e < ne; ++e)
            if (!(edge_absent && edge_absent[e0 + e])) g.add_edge(map[edge_src[e0 + e]], map[edge_dst[e0 + e]], edge_is_ref[e0 + e] != 0, edge_multiplicity[e0 + e]);
        if (!clean(g, c[5])) {
            c[0] = 2;
            c[5] = 0;
            close();
            continue;
        }
        // (a chain's members, for vertex_to_seq: walked before the zip changes the graph is not possible -- the zip decides them; so
        // the members are collected from the merged vertices' first vertex and length along the cleaned graph's one out-edges)
        std::vector<uint32_t> next(g.node.size(), NONE);
        for (uint32_t v = 0; v < g.node.size(); ++v)
            if (g.node[v] && g.out[v].size() == 1) next[v] = g.dst[g.out[v][0]];
        const uint32_t n_conv = (uint32_t)g.node.size();
        c[4] = zip(g);
        g.remove_orphans();
        c[6] = connect(g);
        std::vector<uint32_t> idx(g.node.size(), NONE);
        uint32_t n = 0;
        const size_t b0 = R.bases.size();
        for (uint32_t v = 0; v < g.node.size(); ++v) {
            if (!g.node[v]) continue;
            idx[v] = n++;
            R.base_off.push_back((uint32_t)(R.bases.size() - b0));
            R.first.push_back(g.first[v]);
            R.n_merged.push_back(g.n_merged[v]);
            R.bases.insert(R.bases.end(), g.seq[v].begin(), g.seq[v].end());
            uint32_t at = map[g.first[v]];
            for (uint32_t i = 0; i < g.n_merged[v]; ++i) {
                R.to_seq[v0 + g.first[at]] = idx[v];
                at = at < n_conv ? next[at] : NONE;
            }
        }
        uint32_t n_e = 0;
        for (uint32_t e = 0; e < g.edge.size(); ++e) {
            if (!g.edge[e]) continue;
            ++n_e;
            R.e_src.push_back(idx[g.src[e]]);
            R.e_dst.push_back(idx[g.dst[e]]);
            R.e_ref.push_back(g.is_ref[e]);
            R.e_mult.push_back(g.mult[e]);
        }
        c[1] = n;
        c[2] = n_e;
        c[3] = (uint32_t)(R.bases.size() - b0);
        const uint32_t s = g.find(false), t = g.find(true);
        c[7] = s == NONE ? NONE : idx[s];
        c[8] = t == NONE ? NONE : idx[t];
        close();
    }
    sizes[0] = (uint32_t)R.first.size();
    sizes[1] = (uint32_t)R.e_src.size();
    sizes[2] = (uint32_t)R.bases.size();
}

// ... and hands it over: counts [n_graphs x 9] in phmm_assembly_seqgraph's order of per-graph outputs, then its arrays
extern "C" void assembly_seqgraph_host_copy(uint32_t *counts, uint32_t *v_off, uint32_t *e_off, uint32_t *b_off, uint32_t *base_off, uint32_t *first,
                                            uint32_t *n_merged, uint32_t *e_src, uint32_t *e_dst, uint8_t *e_ref, uint32_t *e_mult, uint8_t *bases,
                                            uint32_t *to_seq) {
    const auto put = [](auto *dst, const auto &v) {
        if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(v[0]));
    };
    put(counts, R.counts);
    put(v_off, R.v_off);
    put(e_off, R.e_off);
    put(b_off, R.b_off);
    put(base_off, R.base_off);
    put(first, R.first);
    put(n_merged, R.n_merged);
    put(e_src, R.e_src);
    put(e_dst, R.e_dst);
    put(e_ref, R.e_ref);
    put(e_mult, R.e_mult);
    put(bases, R.bases);
    put(to_seq, R.to_seq);
}
