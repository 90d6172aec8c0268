// Quality -> probability tables (host copies).  See phmm_tables.cpp.
#pragma once
#include <cstddef>
#include <vector>

namespace phmm {
const std::vector<double> &table_eps();             // [256] 10^(-q/10)
const std::vector<double> &table_jacobian();        // [80001] JacobianLogTable: log10(1 + 10^(-k*1e-4))
const std::vector<double> &table_eps_third();       // [256] eps/3
const std::vector<double> &table_match_to_match();  // [256*257/2] triangular
double initial_condition();                         // 2^1020
double initial_condition_log10();
// PCR indel error model cache, 101 entries (engine.rs:169-193); model 1 Hostile, 2 Aggressive, 3 Conservative
std::vector<unsigned char> pcr_error_model_cache(int model);
// The activity profile's tables (phmm_activity_profile):
// [2][256][ploidy + 1] what update_heterozygous_likelihood adds to genotype i for an entry of (is_alt, quality)
// (haplotype_caller_engine.rs:1497-1507, :1724-1749)
std::vector<double> activity_term_table(unsigned ploidy);
// [256] QualityUtils::qual_to_prob(q) as f32 (quality_utils.rs:82-104)
const std::vector<float> &activity_prob_of_qual();
// BandPassActivityProfile::make_kernel / determine_filter_size (band_pass_activity_profile.rs:82-105); the kernel is empty
// where normalize_sum_to_one's assertion fails
std::vector<double> activity_gaussian_kernel(size_t filter_size, double sigma);
unsigned activity_filter_size(const std::vector<double> &kernel, double min_prob_to_keep_in_filter);
}  // namespace phmm
