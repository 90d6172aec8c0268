// Assembly regions on the device (phmm_regions_kernels.hip): kernel parameters, shared by the kernel file and phmm_regions.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t REG_CLASS_THREADS = 256;   // regions_class_kernel, regions_read_kernel: four waves a block
constexpr uint32_t REG_SCAN_THREADS = 1024;   // regions_scan_kernel
constexpr uint32_t REG_ACTIVE = 1, REG_FORCED = 2, REG_OVER_DEPTH = 4;                 // PHMM_REG_*
constexpr int32_t REG_STATUS_MIN_REGION_SIZE = -1, REG_STATUS_START_PAST_CONTIG = -2;  // PHMM_REG_STATUS_*
constexpr float REG_DENSITY_TOLERANCE = 0.05f;  // PROBABILITY_TOLERANCE_FOR_DENSITY_CHECK

struct RegionsParams {
    uint32_t n_profiles, n_samples, n_reads, n_words;
    uint32_t extension, min_size, max_size, max_prop, max_depth;
    float threshold;
    // per profile
    const float *prob;                // the lists of all profiles
    const uint32_t *first, *len;      // [n_profiles] where a list starts in prob, its states
    const uint64_t *start, *stop, *contig;   // [n_profiles] position of state 0, of the last ADDED state, the contig's length
    const uint32_t *window;           // [n_profiles] (with reads)
    const uint32_t *state_off;        // [n_profiles + 1] host-made prefix of len: a profile's slab
    const uint32_t *word_off;         // [n_profiles + 1] host-made prefix of ceil(len / 64): a profile's words in a plane
    // the three bit planes, bit i of a profile's word i / 64: prob > threshold; the local-minimum test away from the drain
    // point; prob > 0.05
    uint64_t *plane_active, *plane_min, *plane_dense;
    // regions_cut_kernel: the regions of profile k at state_off[k] ...
    uint32_t *slab_first, *slab_len, *slab_flags;   // [states] first state inside the list, states drained, ACTIVE | FORCED
    uint32_t *profile_count;          // [n_profiles]
    int32_t *profile_status;          // [n_profiles]
    uint32_t *profile_region_off;     // [n_profiles + 1]
    // per region (n_regions is known to the host after the scan)
    uint32_t n_regions;
    uint64_t *region_start, *region_end, *region_padded_start, *region_padded_end;
    uint32_t *region_states, *region_flags0, *region_flags, *region_n_reads, *region_profile;
    float *region_density;
    // reads
    const uint32_t *group_read_off;   // [windows * samples + 1]
    const int64_t *read_pos;
    const uint32_t *cigar_off, *cigar, *read_off;
    const uint8_t *quals;
    uint32_t n_groups;
    int64_t *read_end, *read_pmax;    // [n_reads] pos + max(reflen, 1); its running maximum inside the group
    double *read_mean_qual;           // [n_reads]
    uint32_t *pair_lo, *pair_hi, *pair_count;   // [n_regions * n_samples] the candidates [lo, hi) and how many of them overlap
    uint32_t *region_read_off;        // [n_regions * n_samples + 1]
    uint64_t *n_memberships;          // [1] the sum in 64 bits
    uint32_t *region_reads;
};

hipError_t launch_regions_cut(const RegionsParams &p, hipStream_t stream);      // class, cut, scan: profile_region_off
hipError_t launch_regions_spans(const RegionsParams &p, hipStream_t stream);    // spans; reads: ends, maxima, counts, offsets; flags
hipError_t launch_regions_members(const RegionsParams &p, hipStream_t stream);  // region_reads

}  // namespace phmm
