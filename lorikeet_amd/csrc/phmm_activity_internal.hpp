// The activity profile on the device (phmm_activity_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_activity.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "phmm_af_internal.hpp"

namespace phmm {

constexpr uint32_t ACT_THREADS = 256;
constexpr uint32_t ACT_MAX_PLOIDY = 64;          // PHMM_ACTIVITY_MAX_PLOIDY: G = ploidy + 1 <= 65 genotypes of two alleles
constexpr uint32_t ACT_DELETION_QUAL = 30;       // REF_MODEL_DELETION_QUAL (haplotype_caller_engine.rs:111)
constexpr uint32_t ACT_SOFTCLIP_QUAL = 28;       // HQ_BASE_QUALITY_SOFTCLIP_THRESHOLD (:117): qualities above it count
constexpr float ACT_SOFTCLIP_MEAN = 6.0f;        // AVERAGE_HQ_SOFTCLIPS_HQ_BASES_THRESHOLD (:75)
constexpr int32_t ACT_REF_SKIP = -1, ACT_CIGAR_OVERRUN = -2;   // PHMM_ACT_STATUS_*
// a pileup slot: one per base of an M / = / X / D element and one per I element, in CIGAR order
constexpr uint16_t ACT_SLOT_COUNTED = 1, ACT_SLOT_ALT = 2, ACT_SLOT_SOFTCLIPS = 4;   // the quality in bits 8..15

struct ActivityParams {
    uint32_t n_windows, n_samples, n_reads, n_pos, n_profiles;
    uint32_t G;                        // ploidy + 1
    uint32_t bq;
    uint32_t F, max_filter;            // the filter size in use; the stride of the profile lists
    float max_prob_propagation;
    double log10_ploidy;
    double ref_pseudo, indel_pseudo;
    // per window
    const int64_t *win_start;          // [n_windows]
    const int64_t *win_end;            // [n_windows] bound_end: min(start + length, contig length)
    const int64_t *contig_len;         // [n_windows]
    const uint32_t *pos_off;           // [n_windows + 1] positions before the window
    const uint32_t *ref_off;           // [n_windows + 1]
    const uint8_t *ref_bases;
    const uint32_t *group_read_off;    // [n_windows * n_samples + 1]
    int32_t *win_status;               // [n_windows] host-made (the CIGARs are walked there for the workspace bounds)
    // per read
    const uint32_t *read_window;       // [n_reads]
    const int64_t *read_pos;           // [n_reads]
    const int64_t *read_lo;            // [n_reads] first position of the read inside the window's bounds
    const int64_t *read_pmax_end;      // [n_reads] running maximum, inside the read's group, of one past its last position
    const uint32_t *read_span;         // [n_reads] positions the read can put a slot at (0: none)
    const uint32_t *cigar_off;         // [n_reads + 1]
    const uint32_t *cigar;             // (len << 4) | op
    const uint32_t *read_off;          // [n_reads + 1]
    const uint8_t *read_bases, *read_quals;
    const uint64_t *slot_off;          // [n_reads + 1] the read's slots in ws_slot
    const uint64_t *tab_off;           // [n_reads + 1] the read's position table in ws_tab: span + 1 entries
    // tables
    const double *term;                // [2][256][G] the addend of genotype i for a (is_alt, quality) slot
    const float *prob_of_qual;         // [256] (1 - 10^(q / -10)) as f32
    const float *taps;                 // [2 F + 1] the Gaussian kernel as f32
    // workspace
    uint16_t *ws_slot;
    uint32_t *ws_tab;                  // slot index (from the read's first) of the first slot at read_lo + k
    double *read_softclips;            // [n_reads] count_high_quality_soft_clips
    uint32_t *mult;                    // [n_pos] how often a position's band is added
    // per profile
    const uint32_t *prof_window, *prof_pos, *prof_n;   // [n_profiles] window, first position (global index), positions
    uint32_t max_prof_n;               // the most positions of one profile
    // results
    uint32_t *read_counts, *ref_depth, *non_ref_depth;   // [n_pos * n_samples]
    double *gl;                        // [n_pos * n_samples * G]
    int32_t *pl;
    double *softclip_mean;             // [n_pos]
    uint32_t *softclip_count;
    double *qual;
    uint32_t *af_flags;
    float *is_active_prob;
    float *profile_prob;               // profile k's list from prof_pos[k] + k * max_filter, prof_n[k] + max_filter entries
    uint32_t *profile_len;
};

// the slots and position tables of the reads, then the per-position sums and PLs
hipError_t launch_activity_pileup(const ActivityParams &p, hipStream_t stream);
// the uniform event list of the allele-frequency kernel: two alleles, G genotypes, n_samples x G PLs per position
hipError_t launch_activity_events(const ActivityParams &p, uint32_t *work, uint32_t *allele_off, uint32_t *genotype_count,
                                  int32_t *span_del, uint64_t *pl_off, double *prior, uint8_t *kind, hipStream_t stream);
// is_active_prob and the multiplicities, then the band-pass and the list lengths
hipError_t launch_activity_bandpass(const ActivityParams &p, hipStream_t stream);

}  // namespace phmm
