// Genotype assignment on the device (phmm_assign_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_assign.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace phmm {

constexpr uint32_t AS_THREADS = 256;          // four waves: four samples of the event at a time
constexpr uint32_t AS_WAVES = AS_THREADS / 64;
constexpr uint32_t AS_MAX_GENOTYPES = 1024;   // as phmm_genotype_likelihoods (GT_MAX_GENOTYPES)
constexpr uint8_t AS_KIND_SPAN_DEL = 1, AS_KIND_NON_REF = 2;
constexpr uint32_t AS_USE_PLS = 0, AS_USE_POSTERIORS = 1;                       // PHMM_GT_*
constexpr uint8_t AS_UNINFORMATIVE = 1, AS_NON_REF_BEST = 2, AS_REF_ONLY = 4;   // PHMM_GT_SAMPLE_*

// Events are the computed ones (two or more call alleles, at least one sample), densely numbered.
struct AssignParams {
    uint32_t n_samples, ploidy, method;
    const uint32_t *genotype_count;    // [n] G_e over the event's alleles
    const uint32_t *sub_count;         // [n] G'_e over the call's alleles
    const uint32_t *call_off;          // [n + 1] the call's alleles in call_allele / call_kind / call_type
    const uint32_t *call_allele;       // index among the event's alleles, strictly increasing, entry 0 is 0
    const uint8_t *call_kind;          // 0 plain, 1 '*', 2 <NON_REF>
    const uint8_t *call_type;          // AlleleType ordinal: 0 REF, 1 SNP, 2 INDEL (posterior method)
    const uint64_t *pl_off;            // [n] n_samples * G_e PLs, sample-major, at pl + pl_off[e]
    const int32_t *pl;
    const uint8_t *monomorphic;        // [n] the arm of the posterior QUAL update
    const uint32_t *gt_comp_off;       // [G'_max + 1] genotype g's components: gt_comp[gt_comp_off[g] .. gt_comp_off[g + 1])
    const uint32_t *gt_comp;           // allele | count << 16, allele ascending (GenotypeAlleleCounts)
    const uint32_t *rank_off;          // [(ploidy + 1) x rank_stride] the allele-first genotype offset table over the event alleles
    uint32_t rank_stride;
    double het[4], hom[4], diff[4];    // GenotypePriorCalculator's tables by AlleleType, host-made
    double log_10, inv_log_10, log1mexp_threshold;  // (10.0).ln(), its inverse, (0.5).ln(): host-made
    // outputs
    const uint64_t *out_off;           // [n] n_samples * G'_e values, sample-major, in sub_pl / gp / pg
    int32_t *sub_pl;
    double *gp, *pg;                   // posterior method
    int32_t *gt;                       // [n x n_samples x ploidy]
    int32_t *gq;                       // [n x n_samples]
    double *log10_gq;                  // [n x n_samples]
    uint8_t *called, *flags;           // [n x n_samples]
    double *p_no_alt;                  // [n x n_samples] extract_p_no_alt per sample (posterior method; device scratch)
    double *qual_update;               // [n] posterior method
};

hipError_t launch_assign(const AssignParams &p, uint32_t n_events, hipStream_t stream);

}  // namespace phmm
