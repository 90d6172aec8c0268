// The k best haplotype paths of a sequence graph on the device (phmm_paths_kernels.hip): kernel parameters, shared by the
// kernel file and phmm_paths.cpp, and the host arithmetic phmm_paths.cpp and tools/paths_host_check.cpp share.  The graphs
// come as phmm_assembly_seqgraph writes them.  One wave works on a graph; its search tree, queue and marks lie in the
// device-only workspace.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace phmm {

constexpr uint32_t PATHS_OK = 0, PATHS_SKIPPED = 1, PATHS_NO_ENDS = 2, PATHS_NO_PATH = 3, PATHS_CYCLES_STAY = 4, PATHS_WEIGHT_RANGE = 5,
                   PATHS_BUDGET = 6;  // PHMM_PATHS_*
constexpr uint32_t PATHS_NONE = 0xffffffffu, PATHS_EQUALS_REF = 0xfffffffeu, PATHS_MAX_WEIGHT = 1u << 20;
// what the offsets kernel leaves in `fits`: a capacity is too small; everything fits; a total does not fit 32 bits
constexpr uint32_t PATHS_FITS_NO = 0, PATHS_FITS_YES = 1, PATHS_FITS_OVERFLOW = 2;
constexpr int PATHS_THREADS = 64;        // the search: one wave per graph
constexpr int PATHS_EMIT_THREADS = 256;  // the output: four waves per graph, a wave per path
// per graph, in this order (g_counts)
enum { PATHS_C_STATUS, PATHS_C_PATHS, PATHS_C_POPPED, PATHS_C_EDGES_REMOVED, PATHS_C_VERTICES_REMOVED, PATHS_C_PATH_EDGES, PATHS_C_HAP_BYTES, PATHS_COUNTS };
// the planes of the per-vertex workspace, 4 bytes each
enum {
    PATHS_V_OUT,    // CSR: where the vertex's out-edges start in e_csr (one more element than vertices per graph: see csr_off)
    PATHS_V_FILL,   // the counting pass' cursor; then the in-degree the peel counts down; then how often the search extended the vertex
    PATHS_V_LIST,   // the peel's worklist; then the DFS's stack of vertices
    PATHS_V_CURSOR, // the DFS's stack of positions in e_csr
    PATHS_V_SEEN,   // the DFS: 1 + the ordinal of the source whose walk visited the vertex last
    PATHS_VERTEX_WORDS
};

struct PathsParams {
    uint32_t n_graphs, n_regions;               // n_regions 0: no duplicate marks
    const uint32_t *vertex_off, *edge_off, *base_off;   // [n_graphs + 1]
    const uint32_t *vertex_base_off;            // [vertices] inside the graph's bytes
    const uint32_t *edge_src, *edge_dst, *edge_mult;
    const uint8_t *edge_is_ref;
    const uint8_t *bases;
    const uint32_t *pre_status;                 // [n_graphs] what the host decided: PATHS_OK, _SKIPPED, _NO_ENDS, _WEIGHT_RANGE
    const uint32_t *graph_source, *graph_sink;  // [n_graphs], used where vertex_role is nullptr
    const uint8_t *vertex_role;                 // [vertices] or nullptr: bit 0 a source, bit 1 a sink
    uint32_t max_paths, max_nodes;
    const uint64_t *node_off;                   // [n_graphs + 1] the graphs' node pools
    const double *log10_table;                  // L[n] = log10((double)n), n <= the largest total of the call
    const uint32_t *region_ref_off;             // [n_regions + 1] or nullptr
    const uint8_t *ref_bases;
    uint32_t capacity[3];                       // paths, path edges, haplotype bytes the output arrays hold
    // workspace
    uint32_t *w;                                // [PATHS_VERTEX_WORDS][vertices + n_graphs]: a graph's rows start at vertex_off[g] + g
    uint64_t w_stride;
    uint32_t *e_csr;                            // [edges] the out-edges of each vertex, descending
    uint8_t *stack_reach;                       // [vertices] the DFS: a child of the vertex on the stack reached a sink
    uint32_t *n_parent, *n_edge, *n_vertex, *n_len, *n_bytes;   // [nodes] the search tree
    double *n_score;
    uint8_t *n_is_ref;
    uint64_t *q_key;                            // [nodes] the queue: the score's order-preserving key ...
    uint32_t *q_node;                           // ... and the node
    uint32_t *r_node;                           // [nodes] the results in pop order
    // results
    uint8_t *edge_removed, *vertex_removed;     // [edges], [vertices]: in the outputs if asked for, else in the workspace
    uint32_t *g_counts;                         // [n_graphs][PATHS_COUNTS]
    uint32_t *out_off;                          // [3][n_graphs + 1]: paths, path edges, bytes
    uint32_t *fits;                             // [1] PATHS_FITS_*
    double *path_score;                         // [capacity[0]] ...
    uint8_t *path_is_ref;
    uint32_t *path_n_edges, *path_first_equal;  // path_first_equal may be nullptr
    uint32_t *hap_off;                          // [capacity[0] + 1]
    uint32_t *path_edges;                       // [capacity[1]]
    uint8_t *hap_bases;                         // [capacity[2]]
};

// four launches on one stream: the search (one wave per graph), the offsets (one wave), the output (one workgroup per graph) and,
// with region arrays, the duplicate marks (a wave per path)
hipError_t launch_paths(const PathsParams &p, hipStream_t stream);

// ---- host arithmetic (phmm_paths.cpp) -----------------------------------------------------------------------------------------
// a graph's node pool: min(budget, sources + (max_paths - 1) * edges) in 64 bits; max_paths == UINT32_MAX is "no limit"
uint64_t paths_pool_size(uint32_t budget, uint64_t sources, uint32_t max_paths, uint64_t edges);
// L[n] = log10((double)n) for n <= need, by the C library, one call per entry; grows to a power of two of entries, at most
// PATHS_MAX_WEIGHT + 1; returns false if `need` is above PATHS_MAX_WEIGHT
bool paths_grow_log10(std::vector<double> &table, uint64_t need);

}  // namespace phmm
