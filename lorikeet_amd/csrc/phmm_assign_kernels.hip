// Genotype assignment on the device (phmm_assign_genotypes, include/phmm.h): per called event and sample, what the reference's
// GenotypingEngine::calculate_genotypes does with the PLs once the output alleles are known (src/genotype/genotyping_engine.rs:
// 199-235):
//   AlleleSubsettingUtils::subset_alleles (src/model/allele_subsetting_utils.rs:161-296) with subsetted_pl_indices (:310-353),
//   VariantContext::make_genotype_call (src/model/variant_context.rs:309-449) in its UsePLsToAssign and
//   UsePosteriorProbabilities arms, GenotypeLikelihoods::gls_to_pls / get_gq_log10_from_likelihoods
//   (src/genotype/genotype_likelihoods.rs:55-109), GenotypePriorCalculator::get_log10_priors
//   (src/genotype/genotype_prior_calculator.rs:169-199), and the posterior QUAL update (genotyping_engine.rs:216-326).
// One 256-lane workgroup per event:
//   table       lanes over the G' genotypes of the call's alleles: genotype g' is unranked through the composition table
//               (the index order over fewer alleles is a prefix of the order over more), its alleles are mapped to the
//               event's and ranked there with the allele-first offset table -- new index -> old PL index, in LDS; the
//               posterior method adds the genotype's log10 prior beside it
//   samples     one wave per sample, four at a time: the gather through the table into the wave's LDS row (likelihoods
//               pl / -10.0), the first maximum and the best of the rest by butterflies that break ties by the lowest index,
//               the is_informative sum in index order by one lane, the PLs, GQ, GT and type
//   posteriors  prior + likelihood, the first maximum, the scaled values in the LDS row; get_gq_log10_from_posteriors and
//               phred_sum over them with a log10_sum_log10 whose sum is a fixed butterfly (exp10 / log10 are ocml's)
// The default method is integers and single IEEE operations: bit-equal to the reference.  Built with -ffp-contract=off.
#include "../../include/phmm.h"
#include "phmm_assign_internal.hpp"

namespace phmm {
namespace {

constexpr double kSumGlThreshNoCall = -0.1;  // VariantContext::SUM_GL_THRESH_NOCALL (variant_context.rs:109)
constexpr double kF64Epsilon = 2.220446049250313e-16;
constexpr uint32_t kNone = 0xffffffffu;

// Rust's `as i32` on a double: saturating, NaN -> 0
__device__ __forceinline__ int32_t as_i32(double v) {
    if (v != v) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return (int32_t)v;
}

// gls_to_pls (genotype_likelihoods.rs:59-70): min((-10 * (gl - max)).round() as i32, i32::MAX)
__device__ __forceinline__ int32_t to_pl(double gl, double adjust) { return as_i32(round(-10.0 * (gl - adjust))); }

// the maximum over the wave and the lowest index that holds it (every lane gets both)
__device__ __forceinline__ void wave_first_max(double &v, uint32_t &i) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, off);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        if (o > v) v = o;
    }
    return v;
}

// a + b == b + a bit for bit, so every lane ends with the same sum
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// MathUtils::log10_sum_log10 (math_utils.rs:161-197) over f(lo) .. f(hi - 1): the first maximum left out, -inf skipped; the
// sum of the others is each lane's in index order, then a butterfly
template <class F>
__device__ double wave_log10_sum(F f, uint32_t lo, uint32_t hi, uint32_t lane) {
    if (lo >= hi) return -INFINITY;
    double m = -INFINITY;
    uint32_t mi = kNone;
    for (uint32_t g = lo + lane; g < hi; g += 64) {
        const double v = f(g);
        if (mi == kNone || v > m) {
            m = v;
            mi = g;
        }
    }
    wave_first_max(m, mi);
    if (m == -INFINITY) return m;
    double others = 0.0;
    for (uint32_t g = lo + lane; g < hi; g += 64) {
        const double v = f(g);
        if (g != mi && v != -INFINITY) others += exp10(v - m);
    }
    const double sum_tot = 1.0 + wave_sum(others);
    return m + (fabs(sum_tot - 1.0) > kF64Epsilon ? log10(sum_tot) : 0.0);
}

// MathUtils::log10_sum_log10_two_values / _three_values (math_utils.rs:199-222)
__device__ __forceinline__ double sum2(double a, double b) {
    return a > b ? a + log10(1.0 + exp10(b - a)) : b + log10(1.0 + exp10(a - b));
}
__device__ __forceinline__ double sum3(double a, double b, double c) {
    if (a >= b && a >= c) return a + log10(1.0 + exp10(b - a) + exp10(c - a));
    if (b >= c) return b + log10(1.0 + exp10(a - b) + exp10(c - b));
    return c + log10(1.0 + exp10(a - c) + exp10(b - c));
}

// MathUtils::log10_one_minus_pow10 with NaturalLogUtils::log1mexp (math_utils.rs:302-312, natural_log_utils.rs:36-49)
__device__ double log10_one_minus_pow10(double a, const AssignParams &p) {
    if (a > 0.0) return NAN;
    if (a == 0.0) return -INFINITY;
    const double b = a * p.log_10;
    const double l = b < p.log1mexp_threshold ? log1p(-exp(b)) : log(-expm1(b));
    return l * p.inv_log_10;
}

// max(OrderedFloat(0.0), OrderedFloat(v)) and min(OrderedFloat(0.0), OrderedFloat(v)): NaN is the greatest
__device__ __forceinline__ double max0(double v) { return v != v || v >= 0.0 ? v : 0.0; }
__device__ __forceinline__ double min0(double v) { return v < 0.0 ? v : 0.0; }

}  // namespace

__global__ void __launch_bounds__(AS_THREADS) phmm_assign_kernel(AssignParams p) {
    __shared__ uint32_t old_index[AS_MAX_GENOTYPES];
    __shared__ double prior[AS_MAX_GENOTYPES];
    __shared__ double rows[AS_WAVES][AS_MAX_GENOTYPES];

    const uint32_t e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t c0 = p.call_off[e], C = p.call_off[e + 1] - c0;
    const uint32_t G = p.genotype_count[e], Gn = p.sub_count[e], ploidy = p.ploidy, S = p.n_samples;
    const bool posteriors = p.method == AS_USE_POSTERIORS;
    const uint32_t *__restrict__ ca = p.call_allele + c0;
    const uint8_t *__restrict__ kind = p.call_kind + c0;

    // ---- subsetted_pl_indices: new genotype -> its alleles among the call's -> the event's -> the index there ----
    for (uint32_t g = t; g < Gn; g += AS_THREADS) {
        uint32_t index = 0, at = 0;
        double pr = 0.0;
        for (uint32_t c = p.gt_comp_off[g]; c < p.gt_comp_off[g + 1]; ++c) {
            const uint32_t ac = p.gt_comp[c], a = ac & 0xffffu, n = ac >> 16;
            const uint32_t *col = p.rank_off + ca[a];
            for (uint32_t i = 1; i <= n; ++i) index += col[(size_t)(at + i) * p.rank_stride];  // allele_heap_to_index
            at += n;
            if (posteriors) {  // get_log10_priors: sum_over_allele_indices_and_counts, from 0.0 in allele order
                const uint32_t ty = p.call_type[c0 + a];
                pr += n == 2 ? p.hom[ty] : p.het[ty] + p.diff[ty] * (double)(n - 1);
            }
        }
        old_index[g] = index < G ? index : G - 1;  // (never out of range for a validated call)
        prior[g] = g == 0 ? 0.0 : pr;
    }
    __syncthreads();
    bool span_del = false;
    for (uint32_t c = 0; c < C; ++c) span_del = span_del || kind[c] == AS_KIND_SPAN_DEL;

    double *L = rows[wave];
    for (uint32_t base = 0; base < S; base += AS_WAVES) {
        const uint32_t s = base + wave;
        const bool act = s < S;  // (the whole wave alike)
        const size_t es = (size_t)e * S + s;
        double best = -INFINITY, second = -INFINITY;
        uint32_t ibest = kNone;
        if (act) {
            // the subsetted likelihoods pl / -10.0 (get_likelihoods -> pls_to_gls) and max_element_index: the first maximum
            const int32_t *__restrict__ row = p.pl + p.pl_off[e] + (size_t)s * G;
            for (uint32_t g = lane; g < Gn; g += 64) {
                const double v = (double)row[old_index[g]] / -10.0;
                L[g] = v;
                if (ibest == kNone || v > best) {
                    best = v;
                    ibest = g;
                }
            }
            wave_first_max(best, ibest);
            // get_gq_log10_from_likelihoods: the largest of the others (the `>=` scan keeps the last of equals: the same value)
            for (uint32_t g = lane; g < Gn; g += 64)
                if (g != ibest && L[g] >= second) second = L[g];
            second = wave_max(second);
        }
        __syncthreads();
        uint32_t ichosen = ibest;
        bool no_call = false;
        if (act) {
            const uint64_t out = p.out_off[e] + (uint64_t)s * Gn;
            if (!posteriors) {
                // is_informative: the sum in index order, one addition at a time -- lane 0 alone, with the <NON_REF> scan of
                // the best genotype, then both go to the wave
                int verdict = 0;  // bit 0: informative, bit 1: <NON_REF> in the best genotype
                if (lane == 0) {
                    double sum = 0.0;
                    for (uint32_t g = 0; g < Gn; ++g) sum += L[g];
                    verdict = sum < kSumGlThreshNoCall ? 1 : 0;
                    for (uint32_t c = p.gt_comp_off[ibest]; c < p.gt_comp_off[ibest + 1]; ++c)
                        if (kind[p.gt_comp[c] & 0xffffu] == AS_KIND_NON_REF) verdict |= 2;
                }
                verdict = __shfl(verdict, 0);
                const bool informative = (verdict & 1) != 0;
                const bool non_ref = verdict == 3;
                no_call = !informative || non_ref;
                // the chosen index is the first maximum, so the difference is never negative and the normalising arm never runs
                const double qual = best - second;
                const double log10_gq = -1.0 * qual;
                for (uint32_t g = lane; g < Gn; g += 64) p.sub_pl[out + g] = non_ref ? 0 : to_pl(L[g], best);
                if (lane == 0) {
                    p.gq[es] = informative ? as_i32(round(log10_gq * -10.0)) : -1;
                    p.log10_gq[es] = informative ? log10_gq : NAN;
                    p.called[es] = no_call ? 0 : 1;
                    p.flags[es] = (uint8_t)((informative ? 0 : AS_UNINFORMATIVE) | (non_ref ? AS_NON_REF_BEST : 0));
                }
            } else {
                // ebe_add(priors, likelihoods), the first maximum, scale_log_space_array_for_numeric_stability; GP and PG
                double pmax = -INFINITY;
                uint32_t imax = kNone;
                for (uint32_t g = lane; g < Gn; g += 64) {
                    p.sub_pl[out + g] = to_pl(L[g], best);
                    const double v = prior[g] + L[g];
                    L[g] = v;
                    if (imax == kNone || v > pmax) {
                        pmax = v;
                        imax = g;
                    }
                }
                wave_first_max(pmax, imax);
                for (uint32_t g = lane; g < Gn; g += 64) {
                    const double n = L[g] - pmax;
                    L[g] = n;
                    p.gp[out + g] = n == 0.0 ? 0.0 : n * -10.0;
                    p.pg[out + g] = prior[g] == 0.0 ? 0.0 : prior[g] * -10.0;
                }
                ichosen = imax;
            }
        }
        __syncthreads();
        if (act && posteriors) {
            // ---- get_gq_log10_from_posteriors (variant_context.rs:524-571) on the scaled posteriors ----
            auto N = [&](uint32_t g) { return L[g]; };
            const uint32_t b = ichosen;
            double log10_gq;
            if (Gn <= 1) {
                log10_gq = 1.0;
            } else if (Gn == 2) {
                log10_gq = b == 0 ? L[1] : L[0];
            } else if (Gn == 3) {
                log10_gq = min0(sum2(L[b == 0 ? 2 : b - 1], L[b == 2 ? 0 : b + 1]));
            } else if (b == 0) {
                log10_gq = wave_log10_sum(N, 1, Gn, lane);
            } else if (b == Gn - 1) {
                log10_gq = wave_log10_sum(N, 0, b, lane);
            } else {
                log10_gq = min0(sum2(wave_log10_sum(N, 0, b, lane), wave_log10_sum(N, b + 1, Gn, lane)));
            }
            // ---- extract_p_no_alt_with_posteriors (genotyping_engine.rs:282-326) on the GP values ----
            auto gp_of = [&](uint32_t g) { return L[g] == 0.0 ? 0.0 : L[g] * -10.0; };
            auto P = [&](uint32_t g) { return gp_of(g) * -0.1; };
            // QualityUtils::phred_sum (quality_utils.rs:54-72) over the first n values
            auto phred_sum = [&](uint32_t n) -> double {
                if (n == 0) return 1.7976931348623157e308;
                if (n == 1) return gp_of(0);
                if (n == 2) return -10.0 * sum2(P(0), P(1));
                if (n == 3) return -10.0 * sum3(P(0), P(1), P(2));
                return -10.0 * wave_log10_sum(P, 0, n, lane);
            };
            const double all = max0(phred_sum(Gn));
            // with a '*' in the call: posteriors[n] for n in 0 .. ploidy, as the reference indexes them
            const double x = span_del ? max0(phred_sum(ploidy)) - all : gp_of(0) - all;
            if (lane == 0) {
                p.gq[es] = as_i32(round(log10_gq * -10.0));
                p.log10_gq[es] = log10_gq;
                p.called[es] = 1;
                p.flags[es] = 0;
                p.p_no_alt[es] = x;
            }
        }
        if (act) {
            // ---- GT: genotype_allele_counts_at(chosen).as_allele_list, indices into the call's alleles; -1: no call ----
            int32_t *__restrict__ gt = p.gt + es * ploidy;
            const uint32_t k0 = p.gt_comp_off[ichosen], k1 = p.gt_comp_off[ichosen + 1];
            for (uint32_t i = lane; i < ploidy; i += 64) {
                uint32_t a = 0, upto = 0;
                for (uint32_t c = k0; c < k1; ++c) {
                    const uint32_t ac = p.gt_comp[c];
                    a = ac & 0xffffu;
                    upto += ac >> 16;
                    if (i < upto) break;
                }
                gt[i] = no_call ? -1 : (int32_t)a;
            }
        }
        __syncthreads();  // (the wave's row is reused by its next sample)
    }

    // ---- the QUAL update (genotyping_engine.rs:216-235): phred_no_variant_posterior_probability folds the samples in order ----
    if (posteriors && t == 0) {
        double acc = NAN;
        for (uint32_t s = 0; s < S; ++s) {
            const double b = p.p_no_alt[(size_t)e * S + s];
            if (b != b) continue;
            acc = acc != acc ? b : acc + b;
        }
        const double log10_no_variant = acc * -0.1;
        p.qual_update[e] = p.monomorphic[e] ? log10_one_minus_pow10(log10_no_variant, p) + 0.0 : log10_no_variant + 0.0;
    }
}

hipError_t launch_assign(const AssignParams &p, uint32_t n_events, hipStream_t stream) {
    if (!n_events) return hipSuccess;
    hipLaunchKernelGGL(phmm_assign_kernel, dim3(n_events), dim3(AS_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
