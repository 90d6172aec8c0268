// Event discovery on the device (phmm_events_kernels.hip): kernel parameters, shared by the kernel file and phmm_events.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t EV_MAX_REF = 16384;   // reference bases per region: the start-position bitmap lives in LDS (PHMM_EVENTS_MAX_REF)
constexpr uint32_t EV_MAX_HAPS = 512;    // haplotypes per region: the per-locus lists live in LDS (PHMM_EVENTS_MAX_HAPS)
constexpr uint32_t EV_OVERLAP = 3;       // events of one haplotype looked at per locus: at most two can overlap, one to spare
constexpr uint32_t EV_SCAN_THREADS = 1024;
constexpr uint32_t EV_TYPE_NONE = 0, EV_TYPE_SNP = 1, EV_TYPE_MNP = 2, EV_TYPE_INDEL = 3;                  // PHMM_EV_TYPE_*
constexpr int32_t EV_BAD_OPERATOR = -1, EV_BLOCK = -2, EV_MERGE = -3, EV_CIGAR_OVERRUN = -4, EV_ALLELES = -5;  // PHMM_EV_STATUS_*
constexpr uint32_t EV_HAP_IN_TWO_ALLELES = 1;                                                              // PHMM_EV_HAP_IN_TWO_ALLELES

// One event of a haplotype's event map.  Positions are indices into the region's reference bases; the reference allele is
// ref_len of those bases from `start`, the alternate allele alt_len bytes of the haplotype's pool slot from alt_off.
struct HapEvent {
    uint32_t start, end, ref_len, alt_off, alt_len, type;
};

struct EventsParams {
    uint32_t n_regions, n_haps;
    const uint32_t *ref_off;          // [n_regions + 1]
    const uint8_t *ref_bases;
    const uint64_t *ref_start, *win_start, *win_end, *contig_len;   // [n_regions]
    const uint32_t *region_hap_off;   // [n_regions + 1]
    const uint32_t *hap_region;       // [n_haps]
    const uint32_t *hap_off;          // [n_haps + 1]
    const uint8_t *hap_bases;
    const uint32_t *cigar_off;        // [n_haps + 1]
    const uint32_t *cigar;            // (len << 4) | op
    const uint32_t *hap_start;        // [n_haps]
    uint32_t dist, spanning, margin;
    uint32_t cap[6];                  // events, alleles, allele bytes, map entries, haplotype events, haplotype alt bytes
    uint32_t max_loci;                // the stride of the four count arrays
    // workspace
    const uint32_t *ws_ev_off;        // [n_haps + 1] slots of ws_ev / ws_alt: cigar elements + haplotype bases (+ spare)
    HapEvent *ws_ev;
    uint8_t *ws_alt;
    uint32_t *hap_n_ev, *hap_n_alt;   // [n_haps]
    int32_t *hap_status;              // [n_haps]
    uint32_t *loci;                   // region g's loci, ascending, from ref_off[g]
    uint32_t *region_n_loci;          // [n_regions]
    uint32_t *locus_base;             // [n_regions + 1]
    uint32_t *locus_cnt;              // [4 x max_loci] per locus: events (0 / 1), alleles, allele bytes, map entries; then offsets
    uint32_t *hap_dense_ev, *hap_dense_alt;   // [n_haps + 1]
    // results
    uint32_t *required;               // [6]
    int32_t *region_status;           // [n_regions]
    uint32_t *region_event_off;       // [n_regions + 1]
    uint32_t *event_region, *event_allele_off, *event_flags;
    int64_t *event_start, *event_end, *event_loc, *vc_start, *vc_end;
    int32_t *event_hap_allele;
    uint32_t *allele_length, *allele_bases_off;
    uint8_t *allele_kind, *allele_bases;
    int64_t *hap_event_start, *hap_event_end;
    uint32_t *hap_event_ref_length, *hap_event_alt_off, *hap_event_type;
    uint8_t *hap_event_alt;
};

hipError_t launch_events(const EventsParams &p, hipStream_t stream);
hipError_t launch_event_maps(const EventsParams &p, hipStream_t stream);  // the haplotypes' event maps alone, into the workspace

}  // namespace phmm
