// A stand-alone host program for the sanitizers: it calls phmm_assembly_seqgraph's HOST code -- the argument checks, where every
// vertex's bytes lie and the sizing of the sort slots -- on a handle it makes itself, with no device: the launch is a stub that
// reports "no device", so a call with good arguments ends in PHMM_ERR_HIP behind everything the host computes.  Build and run
// (no GPU needed): make -C lorikeet_amd/csrc seqgraph_host_check
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "phmm_seqgraph_internal.hpp"
#include "phmm_staging.hpp"

namespace phmm {
hipError_t launch_seqgraph(const SeqParams &, hipStream_t) { return hipErrorNoDevice; }
}  // namespace phmm
namespace phmm_host {
void set_create_error(const std::string &) {}
}  // namespace phmm_host

namespace {

struct Call {  // two graphs of k = 3: a chain behind a branch with a recovery-made vertex, and a graph without edges
    std::vector<uint32_t> region_ref_off{0, 9, 12}, region_read_off{0, 1, 1}, read_off{0, 6}, k{3};
    std::vector<uint8_t> ref = bytes("ACGCGTCGAGTA"), read = bytes("CGATTT");
    std::vector<uint32_t> vertex_off{0, 5, 6}, edge_off{0, 5, 5}, vertex_seq{0, 0, 0, 1, 0}, vertex_pos{0, 3, 6, 1, 0};
    std::vector<uint32_t> edge_src{0, 0, 2, 3, 4}, edge_dst{1, 2, 3, 4, 1}, mult{1, 2, 3, 4, 5};
    std::vector<uint8_t> is_ref{1, 0, 0, 0, 0};
    std::vector<uint32_t> new_off{0, 1, 1};
    std::vector<uint8_t> new_kmer = bytes("TTA"), vertex_absent = std::vector<uint8_t>(6, 0), edge_absent = std::vector<uint8_t>(5, 0);
    std::vector<uint32_t> flags{0, 0}, capacity{0, 0, 0}, required{7, 7, 7};
    std::vector<uint32_t> per_graph = std::vector<uint32_t>(18, 9), offs = std::vector<uint32_t>(9, 9), to_seq = std::vector<uint32_t>(6, 9);
    bool masks = true, pair = true;
    static std::vector<uint8_t> bytes(const char *s) { return std::vector<uint8_t>(s, s + strlen(s)); }
    int run(phmm_handle *h) {
        return phmm_assembly_seqgraph(h, 2, region_ref_off.data(), ref.data(), region_read_off.data(), read_off.data(), read.data(), nullptr, nullptr, 1,
                                      k.data(), vertex_off.data(), edge_off.data(), vertex_seq.data(), vertex_pos.data(), edge_src.data(), edge_dst.data(),
                                      is_ref.data(), mult.data(), pair ? new_off.data() : nullptr, new_kmer.data(), masks ? vertex_absent.data() : nullptr,
                                      edge_absent.data(), flags.data(), capacity.data(), required.data(), &per_graph[0], &per_graph[2], &per_graph[4],
                                      &per_graph[6], &per_graph[8], &per_graph[10], &per_graph[12], &per_graph[14], &per_graph[16], &offs[0], &offs[3],
                                      &offs[6], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, to_seq.data());
    }
};

int failures = 0;
void expect(bool ok, const char *what, const phmm_handle &h) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s (%s)\n", what, h.err.c_str());
    }
}

}  // namespace

int main() {
    phmm_handle h;
    {
        Call c;  // good arguments: the host pass runs to the end and the stubbed device says no
        const int rc = c.run(&h);
        expect(rc == PHMM_ERR_HIP || rc == PHMM_ERR_NO_DEVICE, "good arguments reach the device", h);
        expect(c.required[0] == 7 && c.to_seq[0] == 9 && c.offs[0] == 9, "nothing written without a device", h);
    }
    {
        Call c;  // a graph of 1 000 edges and one of none: the sort slots are sized per graph
        c.vertex_off = {0, 5, 5};
        c.edge_off = {0, 1000, 1000};
        c.new_off = {0, 1, 1};
        c.edge_src.assign(1000, 0);
        c.edge_dst.assign(1000, 4);
        c.mult.assign(1000, 1);
        c.is_ref.assign(1000, 0);
        c.edge_absent.assign(1000, 0);
        c.vertex_absent.assign(5, 0);
        const int rc = c.run(&h);
        expect(rc == PHMM_ERR_HIP || rc == PHMM_ERR_NO_DEVICE, "many edges reach the device", h);
    }
    const auto refused = [&](const char *what, const char *part, Call &c) {
        const int rc = c.run(&h);
        expect(rc == PHMM_ERR_INVALID_ARG && h.err.find(part) != std::string::npos, what, h);
        expect(c.required[0] == 7 && c.per_graph[0] == 9 && c.to_seq[0] == 9 && c.offs[0] == 9, "nothing written", h);
    };
    { Call c; c.k[0] = 0; refused("k 0", "k[0]", c); }
    { Call c; c.masks = false; refused("one mask", "given together", c); }
    { Call c; c.pair = false; refused("half a pair", "new_vertex_off and new_vertex_kmer", c); }
    { Call c; c.vertex_off[0] = 1; refused("vertex_off", "vertex_off does not start at 0", c); }
    { Call c; c.new_off[1] = 6; refused("new vertices", "more new vertices than vertices", c); }
    { Call c; c.edge_dst[4] = 5; refused("endpoint", "its target 5 reaches n_vertices (5)", c); }
    { Call c; c.vertex_pos[2] = 7; refused("vertex bytes", "leave their sequence", c); }
    { Call c; c.vertex_seq[3] = 2; refused("vertex sequence", "is not one of the region's", c); }
    { Call c; c.vertex_absent[0] = 1; refused("absent endpoint", "it is present and an endpoint is absent", c); }
    { Call c; c.capacity[2] = 4; refused("capacity without arrays", "a capacity above 0 whose arrays are NULL", c); }
    { Call c; c.read_off[0] = 1; refused("read_off", "read_off does not start at 0", c); }
    printf(failures ? "%d check(s) failed\n" : "seqgraph_host_check: ok\n", failures);
    return failures != 0;
}
