// Pruning the read-threading graph on the device (phmm_prune_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_prune.cpp.  The graphs come as phmm_assembly_graph writes them: offsets per graph, endpoints as indices inside the graph.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t PRUNE_OP_CHAINS = 1, PRUNE_OP_CONNECT = 2;              // PHMM_PRUNE_OP_*
constexpr uint32_t PRUNE_HAS_CYCLE = 1, PRUNE_NO_REF_ENDS = 2;             // PHMM_PRUNE_HAS_CYCLE, _NO_REF_ENDS
constexpr uint8_t PRUNE_ABSENT = 1, PRUNE_REMOVED_CHAINS = 2, PRUNE_REMOVED_CONNECT = 4, PRUNE_DANGLING_TAIL = 8,
                  PRUNE_DANGLING_HEAD = 16;                                // PHMM_PRUNE_ABSENT ...
constexpr uint32_t PRUNE_NONE = 0xffffffffu;
constexpr int PRUNE_THREADS = 256;  // one workgroup per graph

// Workspace, device only: 20 bytes per vertex (v_in, v_out, v_inedge, v_ref, v_mark) and 5 per edge (e_ptr, e_bits).
struct PruneParams {
    uint32_t n_graphs, ops;
    const uint32_t *vertex_off, *edge_off;       // [n_graphs + 1]
    const uint32_t *edge_src, *edge_dst;         // [edges]
    const uint8_t *edge_is_ref;
    const uint32_t *edge_mult;                   // the pruning multiplicity
    const uint8_t *vertex_absent, *edge_absent;  // both nullptr or both given
    const uint32_t *prune_factor;                // [n_graphs]
    // workspace
    uint32_t *v_in, *v_out;   // [vertices]  degrees over the edges of the graph at hand (G0, then G1); v_in is counted down by the peeling
    uint32_t *v_inedge;       // [vertices]  an in-edge: THE in-edge where v_in is 1
    uint32_t *v_ref;          // [vertices]  bit 0: a reference edge comes in, bit 1: one goes out (G1)
    uint32_t *v_mark;         // [vertices]  reached (bit 0 forwards, bit 1 backwards) or peeled, by the sweep at hand
    uint32_t *e_ptr;          // [edges]  an ancestor of the edge in its chain; the head once the jumps are done
    uint8_t *e_bits;          // [edges]  bit 0: the edge is a head; bit 1: some edge protects the head's chain; bit 2: peeled
    // results
    uint32_t *graph_flags, *n_chains, *n_chains_removed, *n_vertices_left, *n_edges_left, *ref_source, *ref_sink;  // [n_graphs]
    uint32_t *edge_chain;     // [edges]
    uint8_t *edge_state;      // [edges]
    uint8_t *vertex_state;    // [vertices]
};

hipError_t launch_prune(const PruneParams &p, hipStream_t stream);

}  // namespace phmm
