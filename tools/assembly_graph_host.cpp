// The raw read-threading graph of phmm_assembly_graph as a plain single-threaded host loop over the same arrays, one sample,
// std::unordered_map<std::string, uint32_t> for the vertex map: what tools/assembly_graph_bench.py times beside the device
// call, for scale (no gate).  It threads in the reference's order -- per k and region: every run's scan from 0, then sequence by
// sequence the start, the backward walk and the chain -- and returns per graph the vertices, the edges and the sum of the
// multiplicities, which the tool compares with the device's.
// Built by lorikeet_amd/csrc/Makefile into tools/libassembly_graph_host.so.
#include <cstdint>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

namespace {

using Set = std::unordered_set<std::string>;

void scan(const uint8_t *seq, uint32_t stop, uint32_t k, Set &non_unique) {
    if (stop < k) return;
    Set all;
    for (uint32_t i = 0; i + k <= stop; ++i) {
        std::string kmer((const char *)seq + i, k);
        if (!all.insert(kmer).second) non_unique.insert(std::move(kmer));
    }
}

struct Edge {
    uint32_t source, target, multiplicity;
};

struct Graph {
    uint32_t k;
    Set non_unique;
    std::unordered_map<std::string, uint32_t> map;
    std::string ref_source;
    bool has_source = false;
    std::vector<uint8_t> suffix;                       // per vertex
    std::vector<std::vector<uint32_t>> out, in;        // per vertex, edge indices
    std::vector<Edge> edges;

    uint32_t create(const uint8_t *seq, uint32_t p, const std::string &kmer) {
        suffix.push_back(seq[p + k - 1]);
        out.emplace_back();
        in.emplace_back();
        const uint32_t v = (uint32_t)suffix.size() - 1;
        if (!non_unique.count(kmer)) map.emplace(kmer, v);   // (emplace keeps an entry that is there)
        return v;
    }
    void walk(const uint8_t *seq, uint32_t v) {
        for (int off = (int)k - 2; off >= 0 && in[v].size() == 1; --off) {
            Edge &e = edges[in[v][0]];
            if (suffix[e.source] != seq[off]) break;
            ++e.multiplicity;
            v = e.source;
        }
    }
    void thread(const uint8_t *seq, uint32_t len, uint32_t start, uint32_t stop, bool is_ref) {
        if (len <= start + k) return;
        std::string kmer((const char *)seq + start, k);
        const auto found = map.find(kmer);
        uint32_t v = found == map.end() ? create(seq, start, kmer) : found->second;
        walk(seq, v);
        if (is_ref) ref_source = kmer, has_source = true;
        for (uint32_t p = start + 1; p + k <= stop; ++p) {
            const uint8_t base = seq[p + k - 1];
            uint32_t next = UINT32_MAX;
            for (const uint32_t e : out[v])
                if (suffix[edges[e].target] == base) {
                    ++edges[e].multiplicity;
                    next = edges[e].target;
                    break;
                }
            if (next == UINT32_MAX) {
                kmer.assign((const char *)seq + p, k);
                const auto merge = has_source && kmer == ref_source ? map.end() : map.find(kmer);
                next = merge == map.end() ? create(seq, p, kmer) : merge->second;
                edges.push_back({v, next, 1});
                out[v].push_back((uint32_t)edges.size() - 1);
                in[next].push_back((uint32_t)edges.size() - 1);
            }
            v = next;
        }
    }
};

}  // namespace

extern "C" void assembly_graph_host(uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases, const uint32_t *region_read_off,
                                    const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *read_quals, uint32_t n_k, const uint32_t *ks,
                                    uint32_t min_base_quality, uint32_t *n_vertices, uint32_t *n_edges, uint64_t *multiplicity) {
    for (uint32_t i = 0; i < n_k; ++i) {
        const uint32_t k = ks[i];
        for (uint32_t g = 0; g < n_regions; ++g) {
            const uint8_t *ref = ref_bases + region_ref_off[g];
            const uint32_t ref_len = region_ref_off[g + 1] - region_ref_off[g], o = i * n_regions + g;
            n_vertices[o] = n_edges[o] = 0;
            multiplicity[o] = 0;
            if (ref_len < k) continue;
            Graph graph;
            graph.k = k;
            std::vector<std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> runs;   // read, [start, stop)
            scan(ref, ref_len, k, graph.non_unique);
            for (uint32_t r = region_read_off[g]; r < region_read_off[g + 1]; ++r) {
                const uint8_t *b = read_bases + read_off[r], *q = read_quals + read_off[r];
                const uint32_t len = read_off[r + 1] - read_off[r];
                int64_t last_good = -1;
                for (uint32_t end = 0; end <= len; ++end) {
                    if (end == len || (b[end] & 0xdf) == 'N' || q[end] < min_base_quality) {
                        if (last_good >= 0 && end - last_good >= k) {
                            runs.push_back({r, {(uint32_t)last_good, end}});
                            scan(b, end, k, graph.non_unique);
                        }
                        last_good = -1;
                    } else if (last_good < 0) {
                        last_good = end;
                    }
                }
            }
            graph.thread(ref, ref_len, 0, ref_len, true);
            for (const auto &run : runs) {
                const uint8_t *b = read_bases + read_off[run.first];
                const uint32_t len = read_off[run.first + 1] - read_off[run.first], start = run.second.first, stop = run.second.second;
                for (uint32_t p = start; p + k < stop; ++p)
                    if (!graph.non_unique.count(std::string((const char *)b + p, k))) {
                        graph.thread(b, len, p, stop, false);
                        break;
                    }
            }
            n_vertices[o] = (uint32_t)graph.suffix.size();
            n_edges[o] = (uint32_t)graph.edges.size();
            for (const Edge &e : graph.edges) multiplicity[o] += e.multiplicity;
        }
    }
}
