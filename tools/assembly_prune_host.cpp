// What phmm_assembly_prune computes, as a plain single-threaded host loop over the same arrays, the way a caller walks the
// graphs today: chains from the sources with a queue, a depth-first search for the cycle verdict, two breadth-first searches
// for the connection to the reference ends.  No absent masks.  tools/assembly_prune_bench.py times it beside the device's call
// and compares flags, reference ends, counts and both state arrays.  No device code.
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xffffffffu;
constexpr uint8_t REMOVED_CHAINS = 2, REMOVED_CONNECT = 4, DANGLING_TAIL = 8, DANGLING_HEAD = 16;

struct Graph {
    uint32_t nv, ne;
    const uint32_t *src, *dst, *mult;
    const uint8_t *is_ref;
    uint8_t *e_state, *v_state;
    std::vector<uint32_t> out_off, out_edge, in_off, in_edge;  // adjacency over the edges still there

    void index() {
        out_off.assign(nv + 1, 0);
        in_off.assign(nv + 1, 0);
        for (uint32_t e = 0; e < ne; ++e)
            if (!e_state[e]) {
                ++out_off[src[e] + 1];
                ++in_off[dst[e] + 1];
            }
        for (uint32_t v = 0; v < nv; ++v) {
            out_off[v + 1] += out_off[v];
            in_off[v + 1] += in_off[v];
        }
        out_edge.resize(out_off[nv]);
        in_edge.resize(in_off[nv]);
        std::vector<uint32_t> o(out_off.begin(), out_off.end() - 1), i(in_off.begin(), in_off.end() - 1);
        for (uint32_t e = 0; e < ne; ++e)
            if (!e_state[e]) {
                out_edge[o[src[e]]++] = e;
                in_edge[i[dst[e]]++] = e;
            }
    }
    uint32_t out_degree(uint32_t v) const { return out_off[v + 1] - out_off[v]; }
    uint32_t in_degree(uint32_t v) const { return in_off[v + 1] - in_off[v]; }
};

void reach(const Graph &g, uint32_t start, bool forwards, std::vector<uint8_t> &seen) {
    std::vector<uint32_t> todo{start};
    seen[start] = 1;
    while (!todo.empty()) {
        const uint32_t v = todo.back();
        todo.pop_back();
        const auto &off = forwards ? g.out_off : g.in_off;
        const auto &edge = forwards ? g.out_edge : g.in_edge;
        for (uint32_t i = off[v]; i < off[v + 1]; ++i) {
            const uint32_t w = forwards ? g.dst[edge[i]] : g.src[edge[i]];
            if (!seen[w]) {
                seen[w] = 1;
                todo.push_back(w);
            }
        }
    }
}

}  // namespace

extern "C" void assembly_prune_host(uint32_t n_graphs, const uint32_t *vertex_off, const uint32_t *edge_off, const uint32_t *edge_src,
                                    const uint32_t *edge_dst, const uint8_t *edge_is_ref, const uint32_t *edge_mult, uint32_t ops,
                                    const uint32_t *prune_factor, uint32_t *graph_flags, uint32_t *n_chains, uint32_t *n_chains_removed,
                                    uint32_t *n_vertices_left, uint32_t *n_edges_left, uint32_t *ref_source, uint32_t *ref_sink,
                                    uint8_t *edge_state, uint8_t *vertex_state) {
    for (uint32_t o = 0; o < n_graphs; ++o) {
        Graph g;
        g.nv = vertex_off[o + 1] - vertex_off[o];
        g.ne = edge_off[o + 1] - edge_off[o];
        g.src = edge_src + edge_off[o];
        g.dst = edge_dst + edge_off[o];
        g.mult = edge_mult + edge_off[o];
        g.is_ref = edge_is_ref + edge_off[o];
        g.e_state = edge_state + edge_off[o];
        g.v_state = vertex_state + vertex_off[o];
        for (uint32_t e = 0; e < g.ne; ++e) g.e_state[e] = 0;
        for (uint32_t v = 0; v < g.nv; ++v) g.v_state[v] = 0;
        g.index();
        uint32_t chains = 0, removed = 0, nv_left = g.nv;
        if (ops & 1) {
            // chains from the sources, each chain end queued once
            std::vector<uint32_t> queue;
            std::vector<uint8_t> seen(g.nv, 0);
            for (uint32_t v = 0; v < g.nv; ++v)
                if (!g.in_degree(v)) {
                    queue.push_back(v);
                    seen[v] = 1;
                }
            std::vector<uint32_t> chain, doomed;
            for (size_t at = 0; at < queue.size(); ++at) {
                const uint32_t start = queue[at];
                for (uint32_t i = g.out_off[start]; i < g.out_off[start + 1]; ++i) {
                    chain.assign(1, g.out_edge[i]);
                    uint32_t last = g.dst[g.out_edge[i]];
                    bool low = true;
                    while (g.out_degree(last) == 1 && g.in_degree(last) <= 1 && last != start) {
                        chain.push_back(g.out_edge[g.out_off[last]]);
                        last = g.dst[chain.back()];
                    }
                    for (uint32_t e : chain) low &= g.mult[e] < prune_factor[o] && !g.is_ref[e];
                    ++chains;
                    if (low) {
                        ++removed;
                        doomed.insert(doomed.end(), chain.begin(), chain.end());
                    }
                    if (!seen[last]) {
                        seen[last] = 1;
                        queue.push_back(last);
                    }
                }
            }
            for (uint32_t e : doomed) g.e_state[e] = REMOVED_CHAINS;
            g.index();
            if (g.nv != 1)
                for (uint32_t v = 0; v < g.nv; ++v)
                    if (!g.in_degree(v) && !g.out_degree(v)) {
                        g.v_state[v] = REMOVED_CHAINS;
                        --nv_left;
                    }
        }
        // the reference ends and the dangling ends
        uint32_t source = NONE, sink = NONE;
        for (uint32_t v = 0; v < g.nv; ++v) {
            if (g.v_state[v]) continue;
            bool ref_in = false, ref_out = false;
            for (uint32_t i = g.in_off[v]; i < g.in_off[v + 1]; ++i) ref_in |= g.is_ref[g.in_edge[i]] != 0;
            for (uint32_t i = g.out_off[v]; i < g.out_off[v + 1]; ++i) ref_out |= g.is_ref[g.out_edge[i]] != 0;
            const bool is_source = !ref_in && (ref_out || nv_left == 1), is_sink = !ref_out && (ref_in || nv_left == 1);
            if (is_source && source == NONE) source = v;
            if (is_sink && sink == NONE) sink = v;
            if (!g.out_degree(v) && !is_sink) g.v_state[v] |= DANGLING_TAIL;
            if (!g.in_degree(v) && !is_source) g.v_state[v] |= DANGLING_HEAD;
        }
        // a depth-first search that meets a vertex still on its stack
        uint32_t flags = 0;
        {
            std::vector<uint8_t> colour(g.nv, 0);
            std::vector<std::pair<uint32_t, uint32_t>> stack;
            for (uint32_t root = 0; root < g.nv && !flags; ++root) {
                if (colour[root] || (g.v_state[root] & REMOVED_CHAINS)) continue;
                colour[root] = 1;
                stack.assign(1, {root, g.out_off[root]});
                while (!stack.empty() && !flags) {
                    auto &[v, i] = stack.back();
                    if (i == g.out_off[v + 1]) {
                        colour[v] = 2;
                        stack.pop_back();
                        continue;
                    }
                    const uint32_t w = g.dst[g.out_edge[i++]];
                    if (colour[w] == 1) flags |= 1;
                    else if (!colour[w]) {
                        colour[w] = 1;
                        stack.push_back({w, g.out_off[w]});
                    }
                }
            }
        }
        if (source == NONE || sink == NONE) flags |= 2;
        uint32_t ne_left = 0;
        if ((ops & 2) && !(flags & 2)) {
            std::vector<uint8_t> fwd(g.nv, 0), bwd(g.nv, 0);
            reach(g, source, true, fwd);
            reach(g, sink, false, bwd);
            for (uint32_t v = 0; v < g.nv; ++v)
                if (!(g.v_state[v] & REMOVED_CHAINS) && !(fwd[v] && bwd[v])) {
                    g.v_state[v] |= REMOVED_CONNECT;
                    --nv_left;
                }
            for (uint32_t e = 0; e < g.ne; ++e)
                if (!g.e_state[e] && ((g.v_state[g.src[e]] | g.v_state[g.dst[e]]) & REMOVED_CONNECT)) g.e_state[e] = REMOVED_CONNECT;
        }
        for (uint32_t e = 0; e < g.ne; ++e) ne_left += !g.e_state[e];
        graph_flags[o] = flags;
        n_chains[o] = chains;
        n_chains_removed[o] = removed;
        n_vertices_left[o] = nv_left;
        n_edges_left[o] = ne_left;
        ref_source[o] = source;
        ref_sink[o] = sink;
    }
}
