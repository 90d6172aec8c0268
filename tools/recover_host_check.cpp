// A stand-alone host program for the sanitizers: it calls phmm_assembly_recover's HOST code -- the argument checks, the
// degree pass and the sizing of the working graphs -- on a handle it makes itself, with no device: the launch is a stub that
// reports "no device", so a call with good arguments ends in PHMM_ERR_HIP behind everything the host computes.  Build and run
// (no GPU needed): make -C lorikeet_amd/csrc recover_host_check
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "phmm_recover_internal.hpp"
#include "phmm_staging.hpp"

namespace phmm {
hipError_t launch_recover(const RecoverParams &, uint32_t, hipStream_t) { return hipErrorNoDevice; }
}  // namespace phmm
namespace phmm_host {
void set_create_error(const std::string &) {}
}  // namespace phmm_host

namespace {

struct Call {  // a tail of four vertices on a reference of six, k = 3, as phmm_assembly_graph would lay it out
    phmm_recover_config cfg{PHMM_RECOVER_OP_TAILS | PHMM_RECOVER_OP_HEADS, 1, -1, -1, 1, {25, -50, -110, -6}};
    std::vector<uint32_t> region_ref_off{0, 16}, region_read_off{0, 1}, read_off{0, 8}, k{3};
    std::vector<uint8_t> ref = bytes("ACGTTGCAATCGGATC"), read = bytes("GTTGAACC");
    std::vector<uint32_t> vertex_off{0, 10}, edge_off{0, 9}, vertex_seq{0, 0, 0, 0, 0, 0, 0, 1, 1, 1}, vertex_pos{0, 1, 2, 3, 4, 5, 6, 2, 3, 4};
    std::vector<uint32_t> edge_src{0, 1, 2, 3, 4, 5, 3, 7, 8}, edge_dst{1, 2, 3, 4, 5, 6, 7, 8, 9}, mult{1, 1, 1, 1, 1, 1, 1, 1, 1};
    std::vector<uint8_t> is_ref{1, 1, 1, 1, 1, 1, 0, 0, 0};
    std::vector<uint32_t> factor{0}, capacity{0, 0, 0}, required{7, 7, 7};
    std::vector<uint32_t> per_graph = std::vector<uint32_t>(7, 9), offs = std::vector<uint32_t>(6, 9);
    std::vector<uint8_t> removed = std::vector<uint8_t>(9, 9);
    static std::vector<uint8_t> bytes(const char *s) { return std::vector<uint8_t>(s, s + strlen(s)); }
    int run(phmm_handle *h) {
        return phmm_assembly_recover(h, &cfg, 1, region_ref_off.data(), ref.data(), region_read_off.data(), read_off.data(), read.data(), nullptr,
                                     nullptr, 1, k.data(), vertex_off.data(), edge_off.data(), vertex_seq.data(), vertex_pos.data(), edge_src.data(),
                                     edge_dst.data(), is_ref.data(), mult.data(), mult.data(), nullptr, nullptr, nullptr, factor.data(), capacity.data(),
                                     required.data(), &per_graph[0], &per_graph[1], &per_graph[2], &per_graph[3], &per_graph[4], &per_graph[5],
                                     &per_graph[6], &offs[0], &offs[2], &offs[4], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, nullptr, removed.data());
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
        expect(c.required[0] == 7 && c.removed[0] == 9, "nothing written without a device", h);
    }
    const auto refused = [&](const char *what, const char *part, Call &c) {
        const int rc = c.run(&h);
        expect(rc == PHMM_ERR_INVALID_ARG && h.err.find(part) != std::string::npos, what, h);
        expect(c.required[0] == 7 && c.per_graph[0] == 9 && c.removed[0] == 9, "nothing written", h);
    };
    { Call c; c.cfg.ops = 0; refused("ops 0", "ops is 0", c); }
    { Call c; c.cfg.ops = 8; refused("unknown ops", "unknown bits", c); }
    { Call c; c.cfg.num_pruning_samples = 0; refused("num_pruning_samples", "num_pruning_samples", c); }
    { Call c; c.k[0] = 0; refused("k 0", "k[0]", c); }
    { Call c; c.vertex_off[0] = 1; refused("vertex_off", "vertex_off does not start at 0", c); }
    { Call c; c.edge_dst[8] = 10; refused("endpoint", "its target 10 reaches n_vertices (10)", c); }
    { Call c; c.vertex_pos[9] = 6; refused("vertex bytes", "leave their sequence", c); }
    { Call c; c.vertex_seq[4] = 2; refused("vertex sequence", "is not one of the region's", c); }
    { Call c; c.read_off[1] = 0; c.read_off[0] = 1; refused("read_off", "read_off does not start at 0", c); }
    { Call c; c.cfg.sw_parameters.match_value = 100000000; refused("weights", "reach 1e9", c); }
    printf(failures ? "%d check(s) failed\n" : "recover_host_check: ok\n", failures);
    return failures != 0;
}
