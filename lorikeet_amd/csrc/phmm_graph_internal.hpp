// The raw read-threading graph on the device (phmm_graph_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_graph.cpp.  The k-mer stage's state (phmm_asm_internal.hpp) is an input: prefix hashes, region tables, flag planes.
#pragma once

#include "phmm_asm_internal.hpp"

namespace phmm {

constexpr uint32_t GRAPH_MAX_SAMPLES = 64;         // PHMM_GRAPH_MAX_SAMPLES: distinct read_sample values per region
constexpr uint32_t GRAPH_MAX_PRUNING_SAMPLES = 8;  // PHMM_GRAPH_MAX_PRUNING_SAMPLES
constexpr uint32_t GRAPH_VERTEX_TRACKED = 1, GRAPH_VERTEX_REF_SOURCE = 2;
constexpr unsigned long long GRAPH_NONE = ~0ull;

// A vertex HANDLE is where the vertex lives while its index is unknown: h < n_k x n_slots is a slot of the k-mer stage's
// region table (a uniquely keyed vertex IS its k-mer), n_k x n_slots + t a slot of the trie table, which has the same shape.
// A STAMP is (threading rank of the read << 32) | position: rank 0 is the reference, reads follow in threading order, and the
// runs of a read are consecutive sequences with ascending positions, so stamps order occurrences as threading does.
struct GraphParams {
    AsmParams a;
    uint32_t num_pruning_samples;
    const uint32_t *read_sample;        // [n_reads]  dense inside the region, in order of first appearance (the host)
    const uint32_t *region_n_samples;   // [n_regions]  (the host)
    // workspace, device only
    uint32_t *read_rank, *read_group;   // [n_k x n_reads]  threading rank (1 ..) and group (1 ..) of a read with a run of >= k bases
    uint32_t *order;                    // [n_k x n_reads]  at region_read_off[g] + rank - 1: the read of that rank
    uint32_t *n_yield, *n_groups;       // [n_graphs]  reads with a run; groups, the reference's included
    uint32_t *ref_handle, *read_handle; // [n_k x plane]  ASM_EMPTY = not visited
    uint32_t *ref_edge, *read_edge;     // [n_k x plane]  the edge slot a visited position behind its start traverses
    unsigned long long *trie_claim;     // [n_k x n_slots]  all ones = empty: tag (18) | distance to the anchor (14) | position key (32)
    unsigned long long *v_stamp;        // [2 x n_k x n_slots] by handle, all ones at first: the lowest stamp that lands on the vertex
    unsigned long long *v_in1, *v_in2;  // the two lowest creator stamps among the vertex's in-edges
    uint32_t *v_inedge;                 // the edge slot of v_in1
    uint32_t *v_index;                  // the vertex's index inside its graph
    unsigned long long *e_key;          // [n_k x n_slots]  all ones = empty: source handle << 32 | target handle
    unsigned long long *e_stamp;        // the lowest stamp that traverses the edge
    uint32_t *e_index;                  // the edge's index inside its graph
    uint32_t *seq_n_vertices, *seq_n_edges;        // [n_k x (n_regions + n_reads)]  creators per sequence, then their
    uint32_t *seq_vertex_base, *seq_edge_base;     // exclusive sums in threading order
    // second half: after the host has read the counts
    const uint32_t *vertex_off, *edge_off, *ref_path_off;  // [n_graphs + 1]
    const unsigned long long *count_off;                   // [n_graphs]  where the graph's n_edges x width counts start
    const uint32_t *count_width;                           // [n_graphs]  1 + the region's samples
    uint32_t *counts;                   // per (edge, group) traversals, zeroed by the launcher
    uint32_t *edge_group;               // [edges]  the group of the edge's creator
    // results
    uint32_t *n_vertices, *n_edges, *n_ref_path;           // [n_graphs]
    uint32_t *vertex_seq, *vertex_pos;
    uint8_t *vertex_flags;
    uint32_t *edge_src, *edge_dst, *edge_multiplicity, *edge_pruning_multiplicity;
    uint8_t *edge_is_ref;
    uint32_t *ref_path;
    uint32_t *ref_vertex, *read_vertex;  // [n_k x plane], all ones from the launcher (an empty plane's pointer is nullptr)
    bool want_planes;                    // the vertex planes are asked for
    uint32_t max_edges;                  // the largest n_edges of a graph (the host, second half)
    unsigned long long n_counts;         // the entries of `counts`
};

hipError_t launch_graph_build(const GraphParams &p, hipStream_t stream);  // the k-mer stage, then handles, stamps and counts
hipError_t launch_graph_fill(const GraphParams &p, hipStream_t stream);   // indices, weights, the reference path, the planes

}  // namespace phmm
