// A stand-alone host program for the sanitizers: it calls phmm_assembly_best_paths' HOST code -- the argument checks, what the
// host decides about a graph, the node pools at the 32- and 64-bit edges, the growth of the log10 table and the capacity
// arithmetic of the layout -- on a handle it makes itself, with no device: the launch is a stub that reports "no device", so a
// call with good arguments ends in PHMM_ERR_HIP behind everything the host computes.  Build and run (no GPU needed):
// make -C lorikeet_amd/csrc paths_host_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "phmm_paths_internal.hpp"
#include "phmm_staging.hpp"

namespace phmm {
hipError_t launch_paths(const PathsParams &, hipStream_t) { return hipErrorNoDevice; }
}  // namespace phmm
namespace phmm_host {
void set_create_error(const std::string &) {}
}  // namespace phmm_host

namespace {

struct Call {  // two graphs: a bubble of four vertices and a chain of three; one region per graph
    std::vector<uint32_t> vertex_off{0, 4, 7}, edge_off{0, 4, 6}, base_off{0, 5, 8}, vertex_base_off{0, 1, 3, 4, 0, 1, 2};
    std::vector<uint32_t> src{0, 0, 1, 2, 0, 1}, dst{1, 2, 3, 3, 1, 2}, mult{2, 1, 1, 1, 1, 1};
    std::vector<uint8_t> is_ref{1, 0, 1, 0, 1, 1}, bases = bytes("ACCGTACG"), roles{1, 0, 0, 2, 1, 0, 2};
    std::vector<uint32_t> status{0, 0}, source{0, 0}, sink{3, 2}, region_ref_off{0, 4, 7};
    std::vector<uint8_t> ref = bytes("ACGTACG");
    std::vector<uint32_t> capacity{0, 0, 0}, required{7, 7, 7}, per_graph = std::vector<uint32_t>(10, 9), offs = std::vector<uint32_t>(9, 9);
    std::vector<double> score;
    std::vector<uint8_t> path_is_ref, hap_bases, edge_removed = std::vector<uint8_t>(6, 9), vertex_removed = std::vector<uint8_t>(7, 9);
    std::vector<uint32_t> n_edges, hap_off = std::vector<uint32_t>(1, 9), first_equal, path_edges;
    uint32_t n_graphs = 2, max_paths = 128, max_nodes = 1u << 16, n_regions = 2, n_k = 1;
    bool with_roles = false, with_regions = true, with_first = false, with_ref = true;
    static std::vector<uint8_t> bytes(const char *s) { return std::vector<uint8_t>(s, s + strlen(s)); }
    void room(uint32_t paths, uint32_t edges, uint32_t bytes_) {
        capacity = {paths, edges, bytes_};
        score.assign(paths, 9), path_is_ref.assign(paths, 9), n_edges.assign(paths, 9), hap_off.assign(paths + 1, 9), first_equal.assign(paths, 9);
        path_edges.assign(edges, 9), hap_bases.assign(bytes_, 9);
    }
    int run(phmm_handle *h) {
        const auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
        return phmm_assembly_best_paths(h, n_graphs, vertex_off.data(), edge_off.data(), base_off.data(), vertex_base_off.data(), src.data(), dst.data(),
                                        is_ref.data(), mult.data(), bases.data(), status.data(), with_roles ? nullptr : source.data(),
                                        with_roles ? nullptr : sink.data(), with_roles ? roles.data() : nullptr, max_paths, max_nodes,
                                        with_regions ? n_regions : 0, with_regions ? n_k : 0, with_regions ? region_ref_off.data() : nullptr,
                                        with_regions && with_ref ? ref.data() : nullptr, capacity.data(), required.data(), &per_graph[0], &per_graph[2],
                                        &per_graph[4], &per_graph[6], &per_graph[8], &offs[0], &offs[3], &offs[6], ptr(score), ptr(path_is_ref), ptr(n_edges),
                                        hap_off.data(), with_first || (with_regions && !first_equal.empty()) ? first_equal.data() : nullptr, ptr(path_edges),
                                        ptr(hap_bases), edge_removed.data(), vertex_removed.data());
    }
    bool untouched() const { return required[0] == 7 && per_graph[0] == 9 && offs[0] == 9 && hap_off[0] == 9 && edge_removed[0] == 9 && vertex_removed[0] == 9; }
};

int failures = 0;
void expect(bool ok, const char *what, const std::string &detail = "") {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (%s)\n", what, detail.c_str());
    }
}

}  // namespace

int main() {
    using namespace phmm;
    // ---- the node pools: min(budget, sources + (max_paths - 1) * edges) in 64 bits ---------------------------------------------------
    expect(paths_pool_size(1u << 16, 1, 128, 4) == 1 + 127 * 4, "a small pool");
    expect(paths_pool_size(100, 1, 128, 4) == 100, "the budget bounds the pool");
    expect(paths_pool_size(0xffffffffu, 1, 1, 0xffffffffull) == 1, "max_paths 1: the sources alone");
    expect(paths_pool_size(0xffffffffu, 5, 2, 0xfffffffaull) == 0xffffffffull, "the sum at 2^32 - 1 exactly");
    expect(paths_pool_size(0xffffffffu, 6, 2, 0xfffffffaull) == 0xffffffffull, "the sum one above the budget");
    expect(paths_pool_size(0xffffffffu, 0xffffffffull, 0xfffffffeu, 0xffffffffull) == 0xffffffffull, "a product near 2^64 does not wrap below the budget");
    expect(paths_pool_size(0xffffffffu, 3, 0xffffffffu, 0) == 3, "unlimited paths, no edges");
    expect(paths_pool_size(1000, 3, 0xffffffffu, 1) == 1000, "unlimited paths: the budget");
    // ---- the table ------------------------------------------------------------------------------------------------------------------------
    {
        std::vector<double> t;
        expect(paths_grow_log10(t, 1) && t.size() == 1024 && std::isinf(t[0]) && t[0] < 0 && t[1] == 0.0 && t[10] == 1.0 && t[1000] == std::log10(1000.0), "the first 1 024");
        const double *before = t.data();
        expect(paths_grow_log10(t, 1023) && t.size() == 1024 && t.data() == before, "no growth inside the table");
        expect(paths_grow_log10(t, 1024) && t.size() == 2048 && t[1024] == std::log10(1024.0), "growth at the edge");
        expect(paths_grow_log10(t, PATHS_MAX_WEIGHT) && t.size() == (size_t)PATHS_MAX_WEIGHT + 1 && t[PATHS_MAX_WEIGHT] == std::log10((double)PATHS_MAX_WEIGHT), "the whole range");
        expect(!paths_grow_log10(t, (uint64_t)PATHS_MAX_WEIGHT + 1) && t.size() == (size_t)PATHS_MAX_WEIGHT + 1, "one above the range");
        bool same = true;
        for (size_t n = 1; n < t.size(); ++n) same = same && t[n] == std::log10((double)n);
        expect(same, "every entry is the library's log10");
    }
    phmm_handle h;
    const auto reaches = [&](const char *what, Call &c) {
        const int rc = c.run(&h);
        expect(rc == PHMM_ERR_HIP || rc == PHMM_ERR_NO_DEVICE, what, h.err);
        expect(c.untouched(), "nothing written without a device", what);
    };
    { Call c; reaches("good arguments reach the device", c); expect(h.paths_log10.size() == 1024, "the handle's table holds the first 1 024"); }
    { Call c; c.with_roles = true; reaches("roles in place of the ends", c); }
    { Call c; c.with_regions = false; reaches("no region arrays", c); }
    { Call c; c.room(3, 7, 40); reaches("capacities with their arrays", c); }
    { Call c; c.max_paths = 0xffffffffu; c.max_nodes = 0x7fffffffu; reaches("two pools of 2^31 - 1 nodes: the sum within 32 bits", c); }
    { Call c; c.mult[0] = 1u << 19; c.mult[1] = 1u << 19; reaches("a total of PHMM_PATHS_MAX_WEIGHT", c); expect(h.paths_log10.size() == (size_t)PATHS_MAX_WEIGHT + 1, "the table grew to the range"); }
    { Call c; c.mult[0] = 0xffffffffu; c.mult[1] = 0xffffffffu; reaches("a total beyond 32 bits is a status, not an error", c); }
    { Call c; c.n_graphs = 0; c.with_regions = false; expect(c.run(&h) == PHMM_OK && c.required[0] == 0 && c.offs[0] == 0 && c.hap_off[0] == 0, "no graphs", h.err); }
    const auto refused = [&](const char *what, const char *part, Call &c) {
        const int rc = c.run(&h);
        expect(rc == PHMM_ERR_INVALID_ARG && h.err.find(part) != std::string::npos, what, h.err);
        expect(c.untouched(), "nothing written", what);
    };
    { Call c; c.max_paths = 0; refused("max_paths 0", "max_paths is 0", c); }
    { Call c; c.max_nodes = 0; refused("max_nodes 0", "max_nodes_per_graph is 0", c); }
    { Call c; c.vertex_off[0] = 1; refused("vertex_off", "seq_vertex_off does not start at 0", c); }
    { Call c; c.base_off[2] = 4; refused("base_off", "seq_base_off decreases", c); }
    { Call c; c.dst[5] = 3; refused("endpoint", "its target 3 reaches n_vertices (3)", c); }
    { Call c; c.vertex_base_off[3] = 6; refused("bytes", "is past the graph's bytes (5)", c); }
    { Call c; c.vertex_base_off[2] = 0; refused("bytes descending", "seq_vertex_base_off decreases", c); }
    { Call c; c.source[1] = 3; refused("source", "its source 3 is neither a vertex nor UINT32_MAX", c); }
    { Call c; c.with_roles = true; c.roles[6] = 4; refused("role", "its role 4 is above 3", c); }
    { Call c; c.n_k = 2; refused("n_k x n_regions", "is not n_graphs (2)", c); }
    { Call c; c.with_ref = false; refused("ref_bases", "a required pointer is NULL (ref_bases)", c); }
    { Call c; c.with_regions = false; c.with_first = true; c.first_equal.assign(1, 9); refused("path_first_equal alone", "path_first_equal is given without the region arrays", c); }
    { Call c; c.room(3, 7, 40); c.path_edges.clear(); refused("capacity without arrays", "a capacity above 0 whose arrays are NULL", c); }
    { Call c; c.max_paths = 0xffffffffu; c.max_nodes = 0x80000000u; refused("two pools of 2^31 nodes", "do not fit 32 bits", c); }
    { Call c; c.region_ref_off[1] = 8; refused("region_ref_off", "region_ref_off decreases", c); }
    printf(failures ? "%d check(s) failed\n" : "paths_host_check: ok\n", failures);
    return failures != 0;
}
