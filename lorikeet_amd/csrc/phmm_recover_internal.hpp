// Dangling-end recovery on the device (phmm_recover_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_recover.cpp.  The graphs come as phmm_assembly_graph writes them and phmm_assembly_prune masks them.  One workgroup of
// one wave works on a graph and takes its ends strictly one after the other, on a copy of the graph that it changes as the
// reference changes its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t RECOVER_OP_TAILS = 1, RECOVER_OP_HEADS = 2;             // PHMM_RECOVER_OP_*
constexpr uint32_t RECOVER_TAIL = 0, RECOVER_HEAD = 1;                     // PHMM_RECOVER_KIND_*
enum : uint32_t {                                                          // PHMM_RECOVER_END_*
    RECOVER_NO_PATH = 0, RECOVER_LOOP, RECOVER_AT_REF_END, RECOVER_TOO_SHORT, RECOVER_CIGAR_NOT_OKAY, RECOVER_TOO_FEW_MATCHING,
    RECOVER_WHOLE_INSERTION, RECOVER_TOO_MANY_MISMATCHES, RECOVER_CANNOT_PUSH_REF, RECOVER_CANNOT_EXTEND, RECOVER_MERGED,
    RECOVER_NO_MERGE_POINT, RECOVER_REFERENCE_FAILS
};
constexpr uint32_t RECOVER_NONE = 0xffffffffu;
constexpr int RECOVER_THREADS = 64;            // one wave per graph
constexpr uint32_t RECOVER_MAX_VERTICES = 30000;  // of one graph: a backtrack entry is 16 bits
constexpr uint32_t RECOVER_CIGAR_SHOWN = 4;    // elements of an end's CIGAR that are reported
// per vertex of the working graph (its vertices, then room for the ones extensions make): the summaries and the two stamps
constexpr int RECOVER_VERTEX_WORDS = 10;
// an edge of the working graph carries the bits of xe_flags
constexpr uint8_t RECOVER_EDGE_ABSENT = 1, RECOVER_EDGE_REF = 2;

struct RecoverParams {
    uint32_t n_graphs, n_regions, ops;
    int32_t min_dangling_branch_length, min_matching_bases, max_mismatches_in_dangling_head;
    int32_t w_match, w_mismatch, w_open, w_extend;
    const uint32_t *k;                           // [n_k]; graph g has k[g / n_regions]
    const uint32_t *vertex_off, *edge_off;       // [n_graphs + 1]
    const uint8_t *bases;                        // the reference bases, then the read bases
    const uint32_t *vertex_base;                 // [vertices] where the vertex's k bytes start in `bases`
    const uint32_t *edge_src, *edge_dst, *edge_mult, *edge_pmult;
    const uint8_t *edge_is_ref;
    const uint8_t *vertex_absent, *edge_absent;  // both nullptr or both given
    const uint32_t *prune_factor;                // [n_graphs]
    // the working graph, device only: graph g owns the vertex slots [xv_off[g], xv_off[g+1]) -- its own vertices first -- and
    // the edge slots [xe_off[g], xe_off[g+1]); its ends are written at end slot xend_off[g] on
    const uint32_t *xv_off, *xe_off, *xend_off;  // [n_graphs + 1]
    uint32_t *xv;                                // [RECOVER_VERTEX_WORDS][vertex slots]
    uint8_t *xv_absent;                          // [vertex slots]
    uint32_t *xe_src, *xe_dst, *xe_mult, *xe_pmult;   // [edge slots]
    uint8_t *xe_flags;
    uint64_t xv_total;                           // vertex slots of the call: the stride of xv's planes
    // the aligner's slab of each workgroup: two paths, two strings, the rows and the backtrack matrix
    unsigned char *slab;
    uint64_t slab_stride;
    uint32_t slab_len;                           // the longest path + k the slab has room for
    // results: per graph; per end slot; per new edge slot; per new vertex slot
    uint32_t *g_counts;                          // [n_graphs][8]: tails, tails recovered, heads, heads recovered, new edges, new vertices, rounds, 0
    uint32_t *end_vertex, *end_kind, *end_status, *end_alt_len, *end_ref_len, *end_n_cigar, *end_cigar, *end_edge;
    uint32_t *ne_src, *ne_dst, *ne_mult, *ne_pmult;   // [new edge slots]: graph g's start at xe_off[g] - edge_off[g]
    uint8_t *new_kmer;                           // [new vertex slots][kmer_stride]: graph g's start at xv_off[g] - vertex_off[g]
    uint32_t kmer_stride;
    uint8_t *edge_removed;                       // [edges]
};

// bytes of one workgroup's slab for paths and strings of up to L entries (recover_kernel lays it out in this order)
constexpr size_t recover_slab_bytes(size_t L) {
    return (3 * (L + 1) * 4 + 8 * (L + 2) * 4 + 2 * ((L + 4) / 4 * 4) + 2 * (L + 1) * (L + 1) + 255) / 256 * 256;
}

hipError_t launch_recover(const RecoverParams &p, uint32_t n_blocks, hipStream_t stream);

}  // namespace phmm
