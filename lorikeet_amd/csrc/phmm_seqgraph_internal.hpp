// The zipped sequence graph on the device (phmm_seqgraph_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_seqgraph.cpp.  The graphs come as phmm_assembly_graph writes them, phmm_assembly_prune masks them and
// phmm_assembly_recover extends them.  One workgroup works on a graph; the state of a graph lies in the device-only workspace
// (DESIGN.md (u)).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t SEQ_OK = 0, SEQ_SKIPPED = 1, SEQ_REFERENCE_FAILS = 2;   // PHMM_SEQ_*
constexpr uint32_t SEQ_NONE = 0xffffffffu;
constexpr int SEQ_THREADS = 256;  // one workgroup per graph
// a graph's vertices: an index and a merge time take 31 bits of a sort key
constexpr uint32_t SEQ_MAX_VERTICES = 0x7fffffffu;
// per graph, in this order (g_counts)
enum { SEQ_C_STATUS, SEQ_C_VERTICES, SEQ_C_EDGES, SEQ_C_BASES, SEQ_C_ZIPPED, SEQ_C_CLEAN, SEQ_C_UNCONNECTED, SEQ_C_SOURCE, SEQ_C_SINK, SEQ_COUNTS };
// the planes of the per-vertex workspace, 4 bytes each
enum {
    SEQ_V_FLAGS,    // SEQ_F_*
    SEQ_V_IN, SEQ_V_OUT,   // degrees over the edges of the graph at hand: as converted, then as cleaned
    SEQ_V_REF,      // bit 0: a reference edge comes in, bit 1: one goes out
    SEQ_V_BLEN,     // the bytes the vertex carries: k with in-degree 0 at the conversion, else 1
    SEQ_V_MARK,     // reached by the sweep at hand (clean), kept (bit 0 forwards from the source, bit 1 backwards)
    SEQ_V_PUSH,     // how often the clean step pushes the vertex's edge list
    SEQ_V_HELD,     // that list holds a non-reference edge
    SEQ_V_PRED,     // THE predecessor where the in-degree is 1
    SEQ_V_LINK,     // the predecessor whose chain the vertex continues, or SEQ_NONE
    SEQ_V_ANC0, SEQ_V_ANC1, SEQ_V_DIST0, SEQ_V_DIST1,   // pointer jumping, ping and pong: an ancestor in the chain and its distance
    SEQ_V_CLEN,     // at a chain's start: the vertices of the chain
    SEQ_V_REP,      // the slot of the sequence vertex that holds the vertex's bytes: the chain's first vertex, or the vertex itself
    SEQ_V_ZIN, SEQ_V_ZOUT, SEQ_V_ZREF,   // degrees and reference bits of the zipped graph, on the slots
    SEQ_V_OUTIDX,   // the slot's index in the output graph
    SEQ_V_BYTEOFF,  // where the slot's bytes start inside the graph's bytes
    SEQ_VERTEX_WORDS
};
constexpr uint32_t SEQ_F_GONE = 1, SEQ_F_START = 2, SEQ_F_MERGED = 4, SEQ_F_ALIVE = 8;
// an edge's state: 0 = in the output graph
constexpr uint8_t SEQ_E_ABSENT = 1, SEQ_E_CLEANED = 2, SEQ_E_INTERIOR = 4, SEQ_E_DROPPED = 8;

// Workspace, device only: 84 bytes per vertex (the planes above), 5 per edge (e_state, e_pos) and 16 per sort slot -- a
// graph has as many sort slots as its edge count rounded up to a power of two (at most 32 bytes per edge).
struct SeqParams {
    uint32_t n_graphs, n_regions;
    const uint32_t *k;                           // [n_k]; graph g has k[g / n_regions]
    const uint32_t *vertex_off, *edge_off;       // [n_graphs + 1]
    const uint32_t *key_off;                     // [n_graphs + 1] the graphs' sort slots
    const uint8_t *bases;                        // the reference bases, then the read bases, then the rows of the new vertices
    const uint32_t *vertex_base;                 // [vertices] where the vertex's k bytes start in `bases`
    const uint32_t *edge_src, *edge_dst, *edge_mult;
    const uint8_t *edge_is_ref;
    const uint8_t *vertex_absent, *edge_absent;  // both nullptr or both given
    const uint32_t *graph_flags;                 // [n_graphs] or nullptr
    uint32_t capacity[3];                        // sequence vertices, edges, bytes the output arrays hold
    // workspace
    uint32_t *w;                                 // [SEQ_VERTEX_WORDS][vertices]
    uint64_t v_total;                            // vertices of the call: the stride of w's planes
    uint8_t *e_state;                            // [edges]
    uint32_t *e_pos;                             // [edges] an output edge's index in its graph
    uint64_t *keys;                              // [sort slots][2]
    // results
    uint32_t *g_counts;                          // [n_graphs][SEQ_COUNTS]
    uint32_t *seq_off;                           // [3][n_graphs + 1]: vertices, edges, bytes
    uint32_t *fits;                              // [1] the totals are within `capacity`
    uint32_t *sv_base_off, *sv_first, *sv_n_merged;   // [capacity[0]]
    uint32_t *se_src, *se_dst, *se_mult;         // [capacity[1]]
    uint8_t *se_is_ref;
    uint8_t *seq_bases;                          // [capacity[2]]
    uint32_t *vertex_to_seq;                     // [vertices]
};

// three launches on one stream: the graphs (one workgroup each), the offsets (one workgroup), the output (one workgroup each)
hipError_t launch_seqgraph(const SeqParams &p, hipStream_t stream);

}  // namespace phmm
