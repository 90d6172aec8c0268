// Region trimming on the device (phmm_trim_kernels.hip): kernel parameters, shared by the kernel file and phmm_trim.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "phmm_events_internal.hpp"

namespace phmm {

constexpr uint32_t TRIM_RANK_THREADS = 256;   // trim_order_kernel
constexpr uint32_t TRIM_SCAN_THREADS = 1024;
constexpr uint32_t TRIM_NONE = 0xFFFFFFFFu;
constexpr uint8_t TRIM_VARIATION_SPAN = 1, TRIM_VARIATION_SET = 2;                                   // PHMM_TRIM_VARIATION_*
constexpr int32_t TRIM_FATE_DUPLICATE = -1, TRIM_FATE_CUT_IN_DELETION = -2, TRIM_FATE_EMPTY = -3,     // PHMM_TRIM_FATE_*
                  TRIM_FATE_ALL_INSERTION = -4, TRIM_FATE_NOT_TRIMMED = -5;
constexpr int32_t TRIM_LOCATION = -16, TRIM_LENGTH = -17, TRIM_OPERATOR = -18, TRIM_NOT_FOUND = -19,  // PHMM_TRIM_STATUS_*
                  TRIM_BUILDER = -20, TRIM_REF_ELIMINATED = -21, TRIM_REPEAT_SLICE = -22;

struct TrimParams {
    uint32_t n_regions, n_haps;
    const uint32_t *ref_off;          // [n_regions + 1]
    const uint64_t *ref_start, *active_start, *active_end, *padded_start, *padded_end;   // [n_regions]
    const uint32_t *region_hap_off;   // [n_regions + 1]
    const uint32_t *hap_region;       // [n_haps]
    const uint32_t *hap_off;          // [n_haps + 1]
    const uint8_t *hap_bases;
    const uint32_t *cigar_off;        // [n_haps + 1]
    const uint32_t *cigar;            // (len << 4) | op
    const uint32_t *hap_start;        // [n_haps]
    const uint64_t *loc_start, *loc_end;   // [n_haps]
    const uint8_t *is_ref;            // [n_haps]
    uint32_t pad_snp, pad_indel;
    // the haplotypes' event maps (launch_event_maps)
    const uint32_t *ws_ev_off;        // [n_haps + 1]
    const HapEvent *ws_ev;
    const uint32_t *hap_n_ev;         // [n_haps]
    const int32_t *hap_status;        // [n_haps]
    // workspace: a trimmed haplotype is bases [win_first, win_first + win_len) of its input slot and new_n_cigar elements of
    // its slot of ws_cigar_b; both CIGAR slots are the input's (cigar_off), a trimmed CIGAR never has more elements
    uint32_t *win_first, *win_len, *new_n_cigar, *new_start;   // [n_haps]
    int32_t *hap_panic;               // [n_haps] 0, or the status of the panic this haplotype's trim ends in
    uint32_t *ws_cigar_a, *ws_cigar_b;
    uint32_t *hap_below, *hap_rep;    // [n_haps] surviving haplotypes of the region below this one; its class's representative
    uint32_t *region_n_out;           // [n_regions]
    uint32_t *out_src, *out_len, *out_n_cigar;   // [n_haps] by output index: the input haplotype, its bases, its elements
    // results
    int32_t *region_status;           // [n_regions]
    uint8_t *variation;               // [n_regions]
    uint64_t *variant_start, *variant_end, *span_start, *span_end;                       // [n_regions] the trimmer's two spans
    uint64_t *new_active_start, *new_active_end, *new_padded_start, *new_padded_end;     // [n_regions] trim_with_padded_span
    int32_t *hap_fate;                // [n_haps]
    uint32_t *hap_dup_of;             // [n_haps]
    uint32_t *out_region_hap_off;     // [n_regions + 1]
    uint32_t *out_hap_off, *out_cigar_off;   // [outputs + 1]
    uint8_t *out_bases;
    uint32_t *out_cigar, *out_start, *out_source;
    uint8_t *out_is_ref;
    int32_t *out_region_ref_hap;      // [n_regions]
};

hipError_t launch_trim(const EventsParams &e, const TrimParams &p, hipStream_t stream);

}  // namespace phmm
