// The k-mer stage in front of the read-threading graph on the device (phmm_asm_kernels.hip): kernel parameters, shared by the
// kernel file and phmm_asm.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t ASM_MAX_K_VALUES = 8;        // PHMM_ASM_MAX_K_VALUES
constexpr uint32_t ASM_MAX_K = 255;             // PHMM_ASM_MAX_K
constexpr uint32_t ASM_MAX_REF_BASES = 16384;   // PHMM_ASM_MAX_REF_BASES
constexpr uint32_t ASM_MAX_READ_BASES = 16384;  // PHMM_ASM_MAX_READ_BASES
constexpr uint32_t ASM_LDS_SLOTS = 2048;        // a sequence of up to ASM_LDS_SLOTS / 2 scanned positions keeps its own table in LDS
constexpr uint32_t ASM_THREADS = 256;
constexpr uint32_t ASM_EMPTY = 0xffffffffu;
constexpr uint32_t ASM_READ_KEY = 0x80000000u;  // a position's key: its index in ref_bases, or this | its index in read_bases
// flags per (k, region)
constexpr uint32_t ASM_REF_SHORT = 1, ASM_REF_NON_UNIQUE = 2, ASM_LOW_COMPLEXITY = 4;
// flags per (k, position), and the bits of a slot of the region's table
constexpr uint32_t ASM_NON_UNIQUE = 1, ASM_THREADED = 2, ASM_THREAD_START = 4, ASM_FIRST = 8;
constexpr uint64_t ASM_HASH_BASE = 0x9e3779b97f4a7c15ull;  // odd

struct AsmParams {
    uint32_t n_regions, n_reads, n_k, min_base_quality;
    uint32_t n_ref_bases, n_read_bases;  // the sizes of the two planes: ref_bases and read_bases as the caller gave them
    uint32_t k[ASM_MAX_K_VALUES];
    uint64_t base_pow[ASM_MAX_K_VALUES];  // ASM_HASH_BASE ^ k
    uint64_t fp_mask;                     // the fingerprint bits in use (switch asm_fingerprint_bits; all ones otherwise)
    uint32_t n_slots;                     // region_table_off[n_regions]
    bool want_ids;                        // the id planes are asked for (the pointer of an empty plane is nullptr all the same)
    const uint32_t *region_ref_off;       // [n_regions + 1]
    const uint32_t *region_read_off;      // [n_regions + 1]
    const uint32_t *region_plane_off;     // [n_regions + 1]  read_off[region_read_off[g]]: the region's part of the read plane (the host)
    const uint32_t *region_table_off;     // [n_regions + 1]  the region's slots per k: twice its bases (the host)
    const uint32_t *read_begin;           // [n_reads]  where the read -- its window -- starts in read_bases / read_quals (the host)
    const uint32_t *read_len;             // [n_reads]  (the host)
    const uint32_t *read_region;          // [n_reads]  (the host)
    const uint8_t *ref_bases, *read_bases, *read_quals;
    // workspace, device only
    uint64_t *ref_hash, *read_hash;  // prefix hashes, one entry more than the sequence's bases: reference g's at region_ref_off[g] + g,
                                     // read r's at read_begin[r] + r
    uint16_t *run_end;               // [n_read_bases]  where the usable run that holds the base ends, in the read; the base itself if unusable
    uint32_t *read_scan_stop;        // [n_k x n_reads]  the stop of the read's last run of k bases or more; 0 without one
    uint32_t *read_n_runs;           // [n_k x n_reads]  its runs of k bases or more
    uint8_t *ref_dup, *read_dup;     // [n_k x plane], zeroed by the launcher: 1 = this position met its bytes already in its sequence's own table.
                                     // Of the occurrences of a repeated k-mer ONE, whichever claimed the slot, stays unmarked: good for "any" and
                                     // for the OR into the region's slot, NOT a per-position flag to export
    uint32_t *seq_table;             // the own tables of the sequences that do not fit LDS: [n_k x 2 x (n_ref_bases + n_read_bases)]; nullptr
                                     // when every sequence fits
    unsigned long long *slot_claim;  // [n_k x n_slots], all ones = empty: the fingerprint's low 32 bits above the key of the position that took it
    uint32_t *slot_rep;              // the lowest key with the slot's bytes
    uint32_t *slot_bits;             // ASM_NON_UNIQUE | ASM_THREADED
    uint32_t *slot_id;               // the dense id
    uint32_t *ref_slot, *read_slot;  // [n_k x plane], ASM_EMPTY = not scanned: the slot of the position's k-mer
    // results
    uint32_t *flags, *n_sequences, *n_non_unique, *n_tracked, *n_distinct;  // [n_k x n_regions]
    uint8_t *ref_flags, *read_flags;                                         // [n_k x plane], zeroed by the launcher
    uint32_t *ref_kmer_id, *read_kmer_id;                                    // [n_k x plane], all ones from the launcher; or nullptr
};

hipError_t launch_assembly_kmers(const AsmParams &p, hipStream_t stream);

// Device helpers the k-mer stage (phmm_asm_kernels.hip) and the graph stage (phmm_graph_kernels.hip) share: a sequence and its
// prefix hash, fingerprints, the home slot of a table, byte comparison.
namespace asm_device {

struct Seq {
    const uint8_t *bases;
    uint64_t *hash;   // len + 1 entries
    uint32_t len;
    uint32_t plane;   // where it starts in its plane (ref_bases or read_bases)
    uint32_t region;
};

__device__ inline Seq ref_seq(const AsmParams &p, uint32_t g) {
    const uint32_t o = p.region_ref_off[g];
    return {p.ref_bases + o, p.ref_hash + o + g, p.region_ref_off[g + 1] - o, o, g};
}

__device__ inline Seq read_seq(const AsmParams &p, uint32_t r) {
    const uint32_t o = p.read_begin[r];
    return {p.read_bases + o, p.read_hash + o + r, p.read_len[r], o, p.read_region[r]};
}

__device__ inline uint32_t ref_len(const AsmParams &p, uint32_t g) { return p.region_ref_off[g + 1] - p.region_ref_off[g]; }

__device__ inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// the fingerprint of the k bytes at pos: two loads and a multiply, for any k, from the one prefix hash
__device__ inline uint64_t fingerprint(const AsmParams &p, const uint64_t *hash, uint32_t pos, uint32_t kk) {
    return mix64(hash[pos + p.k[kk]] - hash[pos] * p.base_pow[kk]) & p.fp_mask;
}

__device__ inline uint32_t home_slot(uint64_t fp, uint32_t cap) {
    return __umulhi((uint32_t)(fp >> 32) + (uint32_t)fp * 0x9e3779b1u, cap);
}

__device__ inline bool same_bytes(const uint8_t *a, const uint8_t *b, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

}  // namespace asm_device

}  // namespace phmm
