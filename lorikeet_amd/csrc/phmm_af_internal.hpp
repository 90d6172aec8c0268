// The allele-frequency calculation on the device (phmm_af_kernels.hip): kernel parameters, shared by the kernel file and
// phmm_af.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

namespace phmm {

constexpr uint32_t AF_THREADS = 256;          // four waves: four small events, or one event with many samples
constexpr uint32_t AF_WAVES = AF_THREADS / 64;
constexpr uint32_t AF_MAX_ALLELES = 50;       // GenotypeLikelihoods::MAX_DIPLOID_ALT_ALLELES_THAT_CAN_BE_GENOTYPED
constexpr uint32_t AF_MAX_GENOTYPES = 1024;   // as phmm_genotype_likelihoods (GT_MAX_GENOTYPES)
constexpr uint32_t AF_MAX_ITERATIONS = 10000; // a safety cap the reference does not have (PHMM_AF_NOT_CONVERGED)
constexpr uint32_t AF_BLOCK_PASSES = 8;       // an event whose samples take this many wave passes gets all four waves
constexpr uint8_t AF_KIND_SPAN_DEL = 1, AF_KIND_NON_REF = 2;

struct AfParams {
    uint32_t n_samples;
    uint32_t n_wave_events;            // work[0 .. n_wave_events): one wave each, four per workgroup
    uint32_t n_block_events;           // work[n_wave_events ..): one workgroup each
    const uint32_t *work;              // computed-event indices of this launch
    const uint32_t *allele_off;        // [n_computed + 1] the event's alleles in prior / kind and its per-allele outputs
    const uint32_t *genotype_count;    // [n_computed] G_e
    const int32_t *span_del;           // [n_computed] index of the '*' allele, -1 if none
    const uint64_t *pl_off;            // [n_computed] n_samples * G_e PLs, sample-major, at pl + pl_off[e]
    const int32_t *pl;
    const double *prior;               // per allele: the pseudo count of its prior class
    const uint8_t *kind;               // per allele: 0 plain, 1 '*', 2 <NON_REF>
    const uint32_t *gt_comp_off;       // [G_max + 1] genotype g's components: gt_comp[gt_comp_off[g] .. gt_comp_off[g + 1])
    const uint32_t *gt_comp;           // allele | count << 16, allele ascending (GenotypeAlleleCounts)
    const double *gt_log10_comb;       // [G_max] log10_combination_count, host-made (lgamma)
    const uint64_t *gt_alleles;        // [G_max] bit a: allele a is in the genotype
    const double *neg_log10_alleles;   // [AF_MAX_ALLELES + 1] -log10(A), host-made: the flat start
    double stand_min_conf;
    double log_10, inv_log_10, log1mexp_threshold;  // (10.0).ln(), its inverse, (0.5).ln(): host-made
    // outputs, by computed event / by its alleles
    double *log10_p_no_variant, *log10_p_variant_present, *qual;
    uint32_t *flags, *iterations;
    double *log10_p_absent;
    int64_t *mle_count;
    uint8_t *allele_flags;
};

// K genotypes per lane: 1 (G <= 64), 4 (G <= 256), 8 (G <= 512) or 16 (G <= 1 024)
hipError_t launch_af(const AfParams &p, uint32_t genotypes_per_lane, hipStream_t stream);

// Host side (phmm_af.cpp), shared by phmm_allele_frequency and phmm_activity_profile: what the kernel reads about the genotypes
// of (ploidy, alleles) -- T is genotype_table_of's (component offsets, components) --, the genotypes a lane holds for G, and
// whether an event of G genotypes and n_samples samples takes a workgroup (n_block_events) or a wave (n_wave_events).
struct AfGenotypeTables {
    std::vector<double> log10_comb;          // gt_log10_comb
    std::vector<uint64_t> gt_alleles;
    std::vector<double> neg_log10_alleles;   // [AF_MAX_ALLELES + 1]
};
AfGenotypeTables af_genotype_tables(const std::pair<std::vector<uint32_t>, std::vector<uint32_t>> &T, uint32_t ploidy);
uint32_t af_genotypes_per_lane(uint32_t G);
bool af_is_block_event(uint32_t G, uint32_t n_samples);

}  // namespace phmm
