// Physical phasing on the device (phmm_phase_kernels.hip): kernel parameters, shared by the kernel file and phmm_phase.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t PH_MAX_HAPS = 512;                  // haplotypes per region (PHMM_EVENTS_MAX_HAPS): a set is PH_WORDS x 64 bits
constexpr uint32_t PH_WORDS = PH_MAX_HAPS / 64;
constexpr uint32_t PH_THREADS = 256;
constexpr uint32_t PH_NO_TRIM = 1;                     // PHMM_PH_NO_TRIM
constexpr uint32_t PH_ABORTED = 1;                     // PHMM_PH_ABORTED
constexpr uint8_t PH_KIND_PLAIN = 0, PH_KIND_SPAN_DEL = 1, PH_KIND_NON_REF = 2;   // PHMM_AF_KIND_*

struct PhaseParams {
    uint32_t n_regions, n_events, n_samples, ploidy, flags;
    const uint32_t *region_event_off;   // [n_regions + 1]
    const uint32_t *region_hap_off;     // [n_regions + 1]
    const uint32_t *event_region;       // [n_events]   (made by the host)
    const uint32_t *event_map_off;      // [n_events]   where the event's Nh(region) entries of event_hap_allele start (the host)
    const uint32_t *event_allele_off;   // [n_events + 1]
    const int32_t *event_hap_allele;
    const int64_t *vc_start;            // [n_events]
    const uint32_t *allele_length, *allele_bases_off;
    const uint8_t *allele_kind, *allele_bases;
    const uint32_t *hap_event_off;      // [n_haps + 1]
    const int64_t *hap_event_start;
    const uint32_t *hap_event_alt_off;
    const uint8_t *hap_event_alt;
    const uint32_t *call_allele_off;    // [n_events + 1]
    const uint32_t *call_allele;
    const int32_t *gt;                  // [n_events x n_samples x ploidy] or nullptr
    // workspace, device only
    unsigned long long *region_called;  // [n_regions x PH_WORDS], zeroed by the launcher: the called haplotypes
    unsigned long long *sets;           // [n_events x PH_WORDS]: S_e
    uint32_t *group_leader;             // region g's group c at region_event_off[g] + c: the event that opened it
    // results
    uint32_t *call_rev_trim;            // [n_events]
    int64_t *call_end;                  // [n_events]
    uint32_t *phase_n_haps;             // [n_events]
    uint8_t *hap_in_call;               // as event_hap_allele, or nullptr
    int32_t *phase_group;               // [n_events]
    uint8_t *phase_gt;                  // [n_events]
    int32_t *phase_leader;              // [n_events]
    int64_t *phase_set;                 // [n_events]
    uint32_t *region_alt_haps;          // [n_regions]
    uint32_t *region_phase_flags;       // [n_regions]
    uint8_t *is_phased;                 // [n_events x n_samples] or nullptr (with gt)
    int32_t *gt_phased;                 // [n_events x n_samples x ploidy] or nullptr (with gt)
};

hipError_t launch_phase(const PhaseParams &p, hipStream_t stream);

}  // namespace phmm
