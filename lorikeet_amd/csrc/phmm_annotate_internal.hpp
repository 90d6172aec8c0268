// Annotation of called events (phmm_annotate_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_annotate.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t ANN_THREADS = 256;         // one workgroup per event
constexpr uint32_t ANN_MAX_TILE = 256;        // reads one sweep of the workgroup examines at most (one per lane)
constexpr size_t ANN_LDS_BYTES = 32 * 1024;   // the tile at most: M[C][T] doubles, a column per lane (sized by the batch's largest call)
constexpr uint32_t ANN_MAX_ALLELES = 1024;    // alleles of an event (what phmm_genotype_likelihoods admits at ploidy 1)
constexpr uint32_t ANN_GROUP = 8;             // call alleles whose MQ / BQ histograms (2 x 256 bins each) one pass holds
constexpr uint32_t ANN_AD_SLOTS = 2048;       // AD counters one pass holds: samples per pass = min(ANN_MAX_CHUNK, slots / C)
constexpr uint32_t ANN_MAX_CHUNK = 512;       // samples one pass counts at most
constexpr double ANN_INFORMATIVE = 0.2;       // LOG_10_INFORMATIVE_THRESHOLD (allele_likelihoods.rs:17)
constexpr double ANN_MAX_QD = 45.0;           // MAX_QD_BEFORE_FIXING (variant_annotation.rs:416-424)

struct AnnotateParams {
    uint32_t n_events, n_samples;
    const uint32_t *region_read_off;  // [n_regions + 1]
    const uint32_t *region_hap_off;   // [n_regions + 1]
    const uint64_t *region_lk_off;    // [n_regions]: the region's [read][hap] matrix in `likelihoods` (staged densely)
    const double *likelihoods;
    const uint8_t *keep;              // [n_reads]
    const uint32_t *read_sample;      // [n_reads]
    const int64_t *read_start, *read_end;  // [n_reads] closed spans on the reference
    const uint8_t *mapq;              // [n_reads]
    const uint32_t *event_region;     // [n_events]
    const uint32_t *event_map_off;    // [n_events]: the event's haplotype -> call allele map in event_hap_call
    const int32_t *event_hap_call;    // the index IN THE CALL of the haplotype's allele, -1 = none or not in the call (host-made)
    const uint32_t *call_off;         // [n_events + 1] dense prefix sums of C_e
    const int64_t *event_start, *event_end;  // closed windows
    // BQ: all of these or none (base_q == nullptr)
    const uint32_t *read_off;         // [n_reads + 1] into base_q
    const uint8_t *base_q;
    const uint32_t *cigar_off;        // [n_reads + 1] into cigar (staged densely)
    const uint32_t *cigar;            // BAM-encoded elements
    const int64_t *read_soft_start;   // [n_reads]
    const int64_t *event_pos;         // [n_events]
    const uint8_t *sample_called;     // [n_events * n_samples] or nullptr (every sample called)
    const double *log10_p_error;      // [n_events], NaN: none
    const uint32_t *n_filtered;       // [n_events * n_samples] or nullptr (0)
    int32_t *ad;                      // n_samples x C_e at n_samples * call_off[e], [s][c]
    double *af;                       // alike
    int32_t *dp;                      // [n_events * n_samples]
    uint32_t *ac;                     // [n_events * n_samples]
    uint8_t *mq, *bq;                 // C_e at call_off[e]; bq nullptr without the BQ inputs
    int32_t *info_dp, *qd_depth;      // [n_events]
    double *qd;                       // [n_events]
    uint32_t *flags;                  // [n_events] PHMM_ANN_*
};

hipError_t launch_annotate(const AnnotateParams &p, uint32_t max_call_alleles, hipStream_t stream);

}  // namespace phmm
