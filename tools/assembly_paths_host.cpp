// The work of phmm_assembly_best_paths as a plain single-threaded loop on the host, over the same arrays -- for scale beside the
// device call in tools/assembly_paths_bench.py, not a gate and not a fallback: the library never calls it.  Every array it
// produces must equal the device's (the bench asserts it).  Graphs with one source and one sink, no duplicate marks.
// Build: make -C lorikeet_amd/csrc (tools/libassembly_paths_host.so).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <queue>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xffffffffu, OK = 0, SKIPPED = 1, NO_ENDS = 2, NO_PATH = 3, CYCLES_STAY = 4, WEIGHT_RANGE = 5, BUDGET = 6, MAX_WEIGHT = 1u << 20;

struct Node {
    uint32_t parent, edge, vertex, len;
    double score;
    uint8_t is_ref;
};

struct Out {
    std::vector<uint32_t> counts, path_off{0}, path_edge_off{0}, hap_base_off{0}, n_edges, hap_off{0}, edges;
    std::vector<double> score;
    std::vector<uint8_t> is_ref, bases, edge_removed, vertex_removed;
} out;

std::vector<uint32_t> edges_of(const std::vector<Node> &t, uint32_t n) {
    std::vector<uint32_t> e(t[n].len);
    for (uint32_t i = t[n].len; i; n = t[n].parent) e[--i] = t[n].edge;
    return e;
}

int ordered(double a, double b) {  // OrderedFloat::cmp
    if (a != a || b != b) return (a != a) - (b != b);
    return (a > b) - (a < b);
}

}  // namespace

extern "C" void assembly_paths_host(uint32_t n_graphs, const uint32_t *vertex_off, const uint32_t *edge_off, const uint32_t *base_off,
                                    const uint32_t *vertex_base_off, const uint32_t *src, const uint32_t *dst, const uint8_t *is_ref, const uint32_t *mult,
                                    const uint8_t *bases, const uint32_t *status, const uint32_t *source, const uint32_t *sink, uint32_t max_paths,
                                    uint32_t max_nodes, uint32_t *sizes) {
    out = Out();
    out.edge_removed.assign(edge_off[n_graphs], 0), out.vertex_removed.assign(vertex_off[n_graphs], 0);
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const uint32_t v0 = vertex_off[g], nv = vertex_off[g + 1] - v0, e0 = edge_off[g], ne = edge_off[g + 1] - e0, nb = base_off[g + 1] - base_off[g];
        const uint32_t *S = src + e0, *D = dst + e0, *M = mult + e0;
        uint8_t *e_gone = out.edge_removed.data() + e0, *v_gone = out.vertex_removed.data() + v0;
        uint32_t st = OK, popped = 0, n_e_gone = 0, n_v_gone = 0;
        std::vector<uint32_t> results;
        std::vector<Node> t;
        std::vector<std::vector<uint32_t>> adj(nv);
        for (uint32_t e = ne; e--;) adj[S[e]].push_back(e);  // newest first
        std::vector<uint64_t> total(nv, 0);
        for (uint32_t e = 0; e < ne; ++e) total[S[e]] += M[e];
        if (status && status[g]) st = SKIPPED;
        else if (source[g] == NONE || sink[g] == NONE) st = NO_ENDS;
        else if (nv && *std::max_element(total.begin(), total.end()) > MAX_WEIGHT) st = WEIGHT_RANGE;
        if (st == OK) {
            const uint32_t s = source[g], k = sink[g];
            std::vector<uint32_t> indeg(nv, 0), todo;
            for (uint32_t e = 0; e < ne; ++e) ++indeg[D[e]];
            for (uint32_t v = 0; v < nv; ++v)
                if (!indeg[v]) todo.push_back(v);
            uint32_t peeled = 0;
            while (!todo.empty()) {
                const uint32_t v = todo.back();
                todo.pop_back(), ++peeled;
                for (uint32_t e : adj[v])
                    if (!--indeg[D[e]]) todo.push_back(D[e]);
            }
            if (peeled < nv) {  // the cycle removal as written
                bool found = false, any = false;
                if (s == k) {
                    found = true;
                } else {
                    std::vector<uint8_t> seen(nv, 0);
                    struct Frame {
                        uint32_t v, at;
                        bool reach;
                    };
                    std::vector<Frame> stack{{s, 0, false}};
                    seen[s] = 1;
                    while (!stack.empty()) {
                        Frame &f = stack.back();
                        if (f.at < adj[f.v].size()) {
                            const uint32_t e = adj[f.v][f.at++], c = D[e];
                            if (seen[c]) e_gone[e] = 1, any = true;
                            else if (c == k) f.reach = true;
                            else seen[c] = 1, stack.push_back({c, 0, false});
                        } else {
                            const Frame done = f;
                            stack.pop_back();
                            if (!done.reach) v_gone[done.v] = 1, any = true;
                            if (!stack.empty()) stack.back().reach |= done.reach;
                            else found = done.reach;
                        }
                    }
                }
                if (!found) st = NO_PATH;
                else if (!any) st = CYCLES_STAY;
                if (st != OK) {
                    std::fill(e_gone, e_gone + ne, 0), std::fill(v_gone, v_gone + nv, 0);
                } else {
                    for (uint32_t e = 0; e < ne; ++e) e_gone[e] |= (v_gone[S[e]] | v_gone[D[e]]) << 1, n_e_gone += e_gone[e] != 0;
                    for (uint32_t v = 0; v < nv; ++v) n_v_gone += v_gone[v];
                }
            }
        }
        if (st == OK) {
            const uint32_t s = source[g], k = sink[g];
            const auto less = [&](uint32_t a, uint32_t b) {  // a pops after b
                const int c = ordered(t[a].score, t[b].score);
                if (c) return c < 0;
                return edges_of(t, b) < edges_of(t, a);
            };
            std::priority_queue<uint32_t, std::vector<uint32_t>, decltype(less)> queue(less);
            std::vector<uint32_t> count(nv, 0);
            t.push_back({NONE, NONE, s, 0, 0.0, 1});
            queue.push(0);
            while (!queue.empty() && (max_paths == NONE || results.size() < max_paths) && st == OK) {
                const uint32_t n = queue.top();
                queue.pop(), ++popped;
                const uint32_t v = t[n].vertex;
                if (v == k) {
                    results.push_back(n);
                } else if (!v_gone[v] && (++count[v] < max_paths || max_paths == NONE)) {
                    uint64_t T = 0;
                    for (uint32_t e : adj[v])
                        if (!e_gone[e]) T += M[e];
                    const double lt = T ? std::log10((double)T) : -std::numeric_limits<double>::infinity();
                    for (uint32_t e : adj[v]) {
                        if (e_gone[e]) continue;
                        if (t.size() >= max_nodes) {
                            st = BUDGET;
                            break;
                        }
                        double sc = t[n].score + ((M[e] ? std::log10((double)M[e]) : -std::numeric_limits<double>::infinity()) - lt);
                        if (sc != sc) sc = std::numeric_limits<double>::quiet_NaN();
                        t.push_back({n, e, D[e], t[n].len + 1, sc, (uint8_t)(t[n].is_ref & (is_ref[e0 + e] != 0))});
                        queue.push((uint32_t)t.size() - 1);
                    }
                }
            }
            if (st != OK) results.clear();
        }
        for (uint32_t n : results) {
            const std::vector<uint32_t> e = edges_of(t, n);
            out.score.push_back(t[n].score), out.is_ref.push_back(t[n].is_ref), out.n_edges.push_back(t[n].len);
            out.edges.insert(out.edges.end(), e.begin(), e.end());
            const auto append = [&](uint32_t v) {
                const uint32_t a = vertex_base_off[v0 + v], b = v + 1 < nv ? vertex_base_off[v0 + v + 1] : nb;
                out.bases.insert(out.bases.end(), bases + base_off[g] + a, bases + base_off[g] + b);
            };
            append(source[g]);
            for (uint32_t x : e) append(D[x]);
            out.hap_off.push_back((uint32_t)out.bases.size());
        }
        for (uint32_t x : {st, (uint32_t)results.size(), popped, n_e_gone, n_v_gone}) out.counts.push_back(x);
        out.path_off.push_back((uint32_t)out.score.size()), out.path_edge_off.push_back((uint32_t)out.edges.size()), out.hap_base_off.push_back((uint32_t)out.bases.size());
    }
    sizes[0] = (uint32_t)out.score.size(), sizes[1] = (uint32_t)out.edges.size(), sizes[2] = (uint32_t)out.bases.size();
}

extern "C" void assembly_paths_host_copy(uint32_t *counts, uint32_t *path_off, uint32_t *path_edge_off, uint32_t *hap_base_off, double *score, uint8_t *is_ref,
                                         uint32_t *n_edges, uint32_t *hap_off, uint32_t *edges, uint8_t *bases, uint8_t *edge_removed, uint8_t *vertex_removed) {
    const auto copy = [](auto *to, const auto &from) {
        if (!from.empty()) memcpy(to, from.data(), from.size() * sizeof(from[0]));
    };
    copy(counts, out.counts), copy(path_off, out.path_off), copy(path_edge_off, out.path_edge_off), copy(hap_base_off, out.hap_base_off);
    copy(score, out.score), copy(is_ref, out.is_ref), copy(n_edges, out.n_edges), copy(hap_off, out.hap_off), copy(edges, out.edges), copy(bases, out.bases);
    copy(edge_removed, out.edge_removed), copy(vertex_removed, out.vertex_removed);
}
