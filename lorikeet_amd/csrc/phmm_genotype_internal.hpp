// Per-event genotype likelihoods (phmm_genotype_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_genotype.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t GT_MAX_GENOTYPES = 1024;  // haplotype_caller_genotyping_engine.rs:66 max_genotype_count_to_enumerate
constexpr uint32_t GT_THREADS = 256;         // one workgroup per event
constexpr uint32_t GT_PER_LANE = GT_MAX_GENOTYPES / GT_THREADS;  // genotype accumulators a lane holds
constexpr uint32_t GT_MAX_TILE = 256;        // reads one tile examines at most (one per lane)
constexpr size_t GT_LDS_BYTES = 32 * 1024;   // the tile: M[A][T] + terms[G][T] doubles
constexpr uint32_t GT_JACOBIAN_LAST = 80000; // JacobianLogTable: (MAX_TOLERANCE / TABLE_STEP) entries after the first

struct GenotypeParams {
    uint32_t n_events, n_samples, ploidy;
    const uint32_t *region_read_off;  // [n_regions + 1]
    const uint32_t *region_hap_off;   // [n_regions + 1]
    const uint64_t *region_lk_off;    // [n_regions]: the region's [read][hap] matrix in `likelihoods` (staged densely)
    const double *likelihoods;
    const uint8_t *keep;              // [n_reads]
    const uint32_t *read_sample;      // [n_reads]
    const int64_t *read_start, *read_end;  // [n_reads] closed spans on the reference
    const uint32_t *event_region;     // [n_events]
    const uint32_t *event_allele_off; // [n_events + 1]
    const uint32_t *event_map_off;    // [n_events]: the event's haplotype -> allele map in event_hap_allele
    const int32_t *event_hap_allele;
    const int64_t *event_start, *event_end;  // closed windows
    const uint64_t *event_out_off;    // [n_events]: n_samples * G_e results at this offset of gl / pl
    const uint32_t *genotype_count;   // [n_events] G_e
    const uint32_t *gt_comp_off;      // [G_max + 1]: the components of genotype g are gt_comp[gt_comp_off[g] .. gt_comp_off[g + 1])
    const uint32_t *gt_comp;          // allele | count << 16, allele ascending (GenotypeAlleleCounts)
    const double *log10_k;            // [ploidy + 1]: std::log10(k), host-made
    const double *jacobian;           // [GT_JACOBIAN_LAST + 1] the host's JacobianLogTable (resident)
    double *gl;
    int32_t *pl;
    uint32_t *n_evidence;             // [n_events * n_samples]
};

hipError_t launch_genotype(const GenotypeParams &p, hipStream_t stream);

#ifdef __HIPCC__
// gls_to_pls (genotype_likelihoods.rs:59-70): min((-10 * (gl - max)).round() as i32, i32::MAX), NaN -> 0, `as` saturates.  Shared
// by the kernels that turn GLs into PLs (compile them with -ffp-contract=off).
__device__ __forceinline__ int32_t to_pl(double gl, double adjust) {
    const double v = round(-10.0 * (gl - adjust));
    if (v != v) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return (int32_t)v;
}
#endif

}  // namespace phmm
