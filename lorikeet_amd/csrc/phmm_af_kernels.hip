// The allele-frequency calculation on the device (phmm_allele_frequency, include/phmm.h): per event, what the reference's
// GenotypingEngine::calculate_genotypes computes from the PLs of its samples (src/genotype/genotyping_engine.rs:80-197):
//   AlleleFrequencyCalculator::calculate (src/model/allele_frequency_calculator.rs:198-379) -- the EM loop over
//   effective_allele_counts (:411-450) and Dirichlet::log10_mean_weights until no count moves by more than 0.01, then
//   P(no variant) and P(allele absent) from the final frequencies -- and the output allele subset and QUAL (:132-197,
//   calculate_output_allele_subset :390-449).
// One wave per event, four events per workgroup; an event whose samples need AF_BLOCK_PASSES or more wave passes gets the
// four waves of a workgroup instead, which take every fourth pass and add their partial sums in wave order.
//   lanes       S lanes per sample (S = the power of two >= G, or 64 with K = 4, 8, 16 genotypes per lane when G > 64), 64 / S
//               samples per pass; a genotype's composition, log10 combination count and allele set come from the tables
//   alleles     lane a holds allele a's prior pseudo count, count and log10 frequency (A <= 50 < 64)
//   posterior   (log10 comb. count + PL / -10) + sum of count * log10 f, normalised by log10_sum_log10 over the sample's
//               lanes: the maximum, the sum of 10^(v - max) (exp10) over the others (a fixed butterfly), the |sum - 1| <= EPSILON
//               rule; ties of the maximum add 1.0 each after the first
//   counts      sum over samples of count * 10^posterior, per lane across passes, then one butterfly per allele: the
//               reference folds log10_sum_log10_two_values in sample order instead -- the same number up to rounding
// Every reduction has a fixed shape that depends on the event alone (G, the sample count), so results are bit-identical from
// run to run and independent of the other events of a batch.  Built with -ffp-contract=off.  The reference's pow / log10 are
// ocml's here; the log10 constants, -log10(A) and the combination counts come from the host.
#include "../../include/phmm.h"
#include "phmm_af_internal.hpp"

namespace phmm {
namespace {

constexpr double kConvergence = 0.01;     // THRESHOLD_FOR_ALLELE_COUNT_CONVERGENCE (allele_frequency_calculator.rs:35)
constexpr double kAfEpsilon = 1.0e-10;    // AFCalculationResult::EPSILON
constexpr double kF64Epsilon = 2.220446049250313e-16;

__device__ __forceinline__ double seg_max(double v, uint32_t S) {
    for (uint32_t off = S >> 1; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, (int)off);
        if (o > v) v = o;
    }
    return v;
}

// a + b == b + a bit for bit, so every lane of a segment ends with the same sum
__device__ __forceinline__ double seg_sum(double v, uint32_t S) {
    for (uint32_t off = S >> 1; off > 0; off >>= 1) v += __shfl_xor(v, (int)off);
    return v;
}

__device__ __forceinline__ double readlane(double v, uint32_t lane) { return __shfl(v, (int)lane); }

// MathUtils::log10_sum_log10 (math_utils.rs:161-197) over the values of a segment's lanes that are `in` (every lane calls it)
template <int K>
__device__ __forceinline__ double seg_log10_sum(const double (&v)[K], const bool (&in)[K], uint32_t S) {
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (in[k] && v[k] > m) m = v[k];
    m = seg_max(m, S);
    double others = 0.0, ties = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!in[k] || v[k] == -INFINITY) continue;
        if (v[k] == m) ties += 1.0;
        else others += exp10(v[k] - m);
    }
    others = seg_sum(others, S);
    ties = seg_sum(ties, S);
    if (m == -INFINITY) return m;
    const double sum_tot = 1.0 + (others + (ties - 1.0));
    return m + (fabs(sum_tot - 1.0) > kF64Epsilon ? log10(sum_tot) : 0.0);
}

// MathUtils::log10_one_minus_pow10 with NaturalLogUtils::log1mexp (math_utils.rs:302-312, natural_log_utils.rs:36-49)
__device__ double log10_one_minus_pow10(double a, const AfParams &p) {
    if (a > 0.0) return NAN;
    if (a == 0.0) return -INFINITY;
    const double b = a * p.log_10;
    const double l = b < p.log1mexp_threshold ? log1p(-exp(b)) : log(-expm1(b));
    return l * p.inv_log_10;
}

// The genotypes a lane holds: g_k = j + S k (only K bits live in registers: the rest is read from the tables, which stay in
// the cache).  Their components are walked in allele order with one cursor each, so a loop over the alleles a = 0, 1, ...
// meets every component of every genotype once, in the reference's order.
template <int K>
__device__ void af_event(const AfParams &p, uint32_t e, uint32_t nw, uint32_t wi, double *xchg) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t a_base = p.allele_off[e], A = p.allele_off[e + 1] - a_base, G = p.genotype_count[e];
    const int32_t sd = p.span_del[e];
    uint32_t S = 64;
    if (K == 1) {
        S = 1;
        while (S < G) S <<= 1;
    }
    const uint32_t spp = 64 / S, j = lane % S, slot = lane / S;
    const uint32_t n_samples = p.n_samples, n_passes = (n_samples + spp - 1) / spp;
    const int32_t *__restrict__ pl = p.pl + p.pl_off[e];

    uint32_t has = 0;  // bit k: g_k < G
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (j + S * (uint32_t)k < G) has |= 1u << k;
    auto gk = [&](int k) { return j + S * (uint32_t)k; };
    const bool is_allele = lane < A;
    const double prior = is_allele ? p.prior[a_base + lane] : 0.0;
    double log10_f = is_allele ? p.neg_log10_alleles[A] : 0.0;
    double count = 0.0;

    // the sum over the event's waves of a value lane a holds (block mode), in wave order; every wave gets the total
    auto combine = [&](double v) -> double {
        if (nw == 1) return v;
        xchg[wi * 64 + lane] = v;
        __syncthreads();
        double t = xchg[lane];
        for (uint32_t w = 1; w < nw; ++w) t += xchg[w * 64 + lane];
        __syncthreads();
        return t;
    };
    // the unnormalised log10 posterior of each of the lane's genotypes for sample s (:126-139, likelihoods pl / -10.0)
    auto unnormalised = [&](const double (&prior_term)[K], uint32_t s, bool (&in)[K], double (&v)[K]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            in[k] = ((has >> k) & 1u) && s < n_samples;
            v[k] = -INFINITY;
            if (in[k]) {
                const uint32_t g = gk(k);
                v[k] = (p.gt_log10_comb[g] + (double)pl[(size_t)s * G + g] / -10.0) + prior_term[k];
            }
        }
    };
    // sum over components of count * log10 f[allele], from 0.0 in allele order (sum_over_allele_indices_and_counts)
    auto prior_terms = [&](double (&t)[K]) {
        uint32_t cur[K], end[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            t[k] = 0.0;
            cur[k] = ((has >> k) & 1u) ? p.gt_comp_off[gk(k)] : 0;
            end[k] = ((has >> k) & 1u) ? p.gt_comp_off[gk(k) + 1] : 0;
        }
        for (uint32_t a = 0; a < A; ++a) {
            const double fa = readlane(log10_f, a);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (cur[k] < end[k]) {
                    const uint32_t ac = p.gt_comp[cur[k]];
                    if ((ac & 0xffffu) == a) {
                        t[k] += (double)(ac >> 16) * fa;
                        ++cur[k];
                    }
                }
            }
        }
    };

    // ---- the EM loop (:218-243) ----
    uint32_t it = 0;
    double diff = INFINITY;
    while (diff > kConvergence && it < AF_MAX_ITERATIONS) {
        double pt[K], P[K];
        prior_terms(pt);
#pragma unroll
        for (int k = 0; k < K; ++k) P[k] = 0.0;
        for (uint32_t pass = wi; pass < n_passes; pass += nw) {
            bool in[K];
            double v[K];
            unnormalised(pt, pass * spp + slot, in, v);
            const double norm = seg_log10_sum(v, in, S);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (in[k]) P[k] += exp10(v[k] - norm);
        }
        // effective_allele_counts: lane a gets sum over samples and genotypes of count_a(g) * posterior(g)
        double fresh = 0.0;
        {
            uint32_t cur[K], end[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                cur[k] = ((has >> k) & 1u) ? p.gt_comp_off[gk(k)] : 0;
                end[k] = ((has >> k) & 1u) ? p.gt_comp_off[gk(k) + 1] : 0;
            }
            for (uint32_t a = 0; a < A; ++a) {
                double c = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (cur[k] < end[k]) {
                        const uint32_t ac = p.gt_comp[cur[k]];
                        if ((ac & 0xffffu) == a) {
                            c += (double)(ac >> 16) * P[k];
                            ++cur[k];
                        }
                    }
                }
                c = seg_sum(c, 64);
                if (lane == a) fresh = c;
            }
        }
        fresh = combine(fresh);
        // max |old - new| (ebe_subtract, OrderedFloat max), then the Dirichlet mean weights of prior + counts
        diff = seg_max(is_allele ? fabs(count - fresh) : 0.0, 64);
        count = fresh;
        const double posterior = prior + count;
        double total = 0.0;
        for (uint32_t a = 0; a < A; ++a) total += readlane(posterior, a);
        log10_f = is_allele ? log10(posterior / total) : 0.0;
        ++it;
    }

    // ---- P(no variant), P(allele absent) from the final frequencies (:245-350) ----
    const bool biallelic_shortcut = A == 2 && sd < 0;
    const uint64_t ref_or_sd = sd < 0 ? 1ull : (1ull | 1ull << sd);
    double pnv = 0.0, absent = 0.0;
    {
        double pt[K];
        prior_terms(pt);
        for (uint32_t pass = wi; pass < n_passes; pass += nw) {
            const uint32_t s = pass * spp + slot;
            const bool leader = j == 0 && s < n_samples;
            bool in[K];
            double v[K];
            unnormalised(pt, s, in, v);
            const double norm = seg_log10_sum(v, in, S);
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] -= norm;
            if (sd < 0) {
                if (leader) pnv += v[0];  // genotype 0 is lane j == 0, k == 0
            } else {
                // genotype_indices_with_only_ref_and_span_del: the genotypes over {ref, '*'} alone; capped at 0
                bool nv[K];
#pragma unroll
                for (int k = 0; k < K; ++k) nv[k] = in[k] && (p.gt_alleles[gk(k)] & ~ref_or_sd) == 0;
                const double r = seg_log10_sum(v, nv, S);
                if (leader) pnv += r < 0.0 ? r : 0.0;
            }
            if (biallelic_shortcut) continue;
            for (uint32_t a = 1; a < A; ++a) {
                bool ab[K];
#pragma unroll
                for (int k = 0; k < K; ++k) ab[k] = in[k] && !((p.gt_alleles[gk(k)] >> a) & 1ull);
                const double r = seg_log10_sum(v, ab, S);
                const double x = seg_sum(leader ? (r < 0.0 ? r : 0.0) : 0.0, 64);
                if (lane == a) absent += x;
            }
        }
    }
    pnv = combine(seg_sum(pnv, 64));
    absent = combine(absent);
    if (biallelic_shortcut) absent = pnv;
    if (wi != 0) return;

    // ---- the output subset and QUAL (genotyping_engine.rs:132-197, :376-449) ----
    const uint8_t kind = is_allele ? p.kind[a_base + lane] : 0;
    const bool alt = is_allele && lane > 0;
    const bool plausible = alt && (absent + kAfEpsilon) < p.stand_min_conf * -0.1;
    const bool output = alt && (plausible || (A == 2 && kind == AF_KIND_NON_REF)) && kind != AF_KIND_SPAN_DEL;
    const bool monomorphic = __ballot(plausible && kind != AF_KIND_SPAN_DEL) == 0;
    const uint64_t outs = __ballot(output);
    const uint32_t first_out = outs ? (uint32_t)__ffsll((unsigned long long)outs) - 1 : 0;
    const int first_kind = __shfl((int)kind, (int)first_out);
    if (is_allele) {
        const uint32_t o = a_base + lane;
        p.log10_p_absent[o] = lane == 0 ? 0.0 : absent;
        p.mle_count[o] = (int64_t)round(count);
        p.allele_flags[o] = (uint8_t)((plausible ? PHMM_AF_ALLELE_PLAUSIBLE : 0u) | (output ? PHMM_AF_ALLELE_OUTPUT : 0u));
    }
    if (lane == 0) {
        const double present = log10_one_minus_pow10(pnv, p);
        const double log10_confidence = monomorphic ? present + 0.0 : pnv + 0.0;
        const double qual = (-10.0 * log10_confidence) + 0.0;
        const bool passes_call = qual >= p.stand_min_conf;
        const bool passes_emit = !monomorphic && passes_call;
        const bool called = passes_emit || (outs != 0 && first_kind == AF_KIND_NON_REF);
        p.log10_p_no_variant[e] = pnv;
        p.log10_p_variant_present[e] = present;
        p.qual[e] = qual;
        p.iterations[e] = it;
        p.flags[e] = (called ? PHMM_AF_CALLED : 0u) | (passes_call ? 0u : PHMM_AF_LOW_QUAL) | (monomorphic ? PHMM_AF_MONOMORPHIC : 0u) |
                     (diff > kConvergence ? PHMM_AF_NOT_CONVERGED : 0u);
    }
}

}  // namespace

template <int K>
__global__ void __launch_bounds__(AF_THREADS) phmm_af_kernel(AfParams p) {
    __shared__ double xchg[AF_WAVES * 64];
    const uint32_t wave = threadIdx.x >> 6, wave_groups = (p.n_wave_events + AF_WAVES - 1) / AF_WAVES;
    if (blockIdx.x < wave_groups) {
        const uint32_t i = blockIdx.x * AF_WAVES + wave;
        if (i < p.n_wave_events) af_event<K>(p, p.work[i], 1, 0, xchg);
    } else {
        af_event<K>(p, p.work[p.n_wave_events + (blockIdx.x - wave_groups)], AF_WAVES, wave, xchg);
    }
}

hipError_t launch_af(const AfParams &p, uint32_t genotypes_per_lane, hipStream_t stream) {
    const uint32_t grid = (p.n_wave_events + AF_WAVES - 1) / AF_WAVES + p.n_block_events;
    if (!grid) return hipSuccess;
    switch (genotypes_per_lane) {
        case 1: hipLaunchKernelGGL(phmm_af_kernel<1>, dim3(grid), dim3(AF_THREADS), 0, stream, p); break;
        case 4: hipLaunchKernelGGL(phmm_af_kernel<4>, dim3(grid), dim3(AF_THREADS), 0, stream, p); break;
        case 8: hipLaunchKernelGGL(phmm_af_kernel<8>, dim3(grid), dim3(AF_THREADS), 0, stream, p); break;
        case 16: hipLaunchKernelGGL(phmm_af_kernel<16>, dim3(grid), dim3(AF_THREADS), 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace phmm
