// Per-event genotype likelihoods on the device (phmm_genotype_likelihoods, include/phmm.h): for every variant event of a
// region and every sample, what the reference's assign_genotype_likelihoods computes from the region's likelihood matrix
// (src/haplotype/haplotype_caller_engine.rs:1379):
//   AlleleLikelihoods::marginalize (allele_likelihoods.rs:693-740) -> retain_evidence with the genotyping engine's overlap
//   predicate (haplotype_caller_genotyping_engine.rs:759-768) -> GenotypeLikelihoodCalculator::genotype_likelihoods
//   (genotype_likelihood_calculator.rs:308-580) -> GenotypeLikelihoods::gls_to_pls (genotype_likelihoods.rs:55-78).
// One 256-lane workgroup per event.  The event's reads go through LDS in tiles of T reads, in region order:
//   1. a lane per read tests keep / sample / overlap; the survivors are compacted order-preserving (ballot + prefix count)
//      and each marginalizes its row into M[a][j] (strict >, haplotypes in order, from -inf: the reference's loop);
//   2. lanes over (read, genotype) pairs write the per-read term of the genotype (one, two or many components) to LDS --
//      the Jacobian lookups of different reads are independent here;
//   3. a lane per genotype adds its terms in read order into an accumulator that stays in registers across tiles.
// Every step is one IEEE operation, a table lookup or a comparison (built with -ffp-contract=off), so the results are the
// reference's bits.  log10(k) and the Jacobian table come from the host (std::log10); the device log10 is never used.
#include "phmm_genotype_internal.hpp"

namespace phmm {
namespace {

constexpr double kMaxTolerance = 8.0;              // JacobianLogTable::MAX_TOLERANCE (math_utils.rs:481-485)
constexpr double kInvStep = 1.0 / 0.0001;          // JacobianLogTable::INV_STEP

// JacobianLogTable::get: (difference * INV_STEP).round() as usize -- round half away from zero, a negative value saturates to 0
__device__ __forceinline__ double jacobian_get(const double *__restrict__ table, double diff) {
    double k = round(diff * kInvStep);
    if (!(k > 0.0)) k = 0.0;
    if (k > (double)GT_JACOBIAN_LAST) k = (double)GT_JACOBIAN_LAST;  // (never: diff < MAX_TOLERANCE)
    return table[(uint32_t)k];
}

// MathUtils::approximate_log10_sum_log10 (math_utils.rs:314-332)
__device__ __forceinline__ double approx_sum2(const double *__restrict__ table, double a, double b) {
    if (a > b) {
        const double t = a;
        a = b;
        b = t;
    }
    if (a == -INFINITY) return b;
    const double diff = b - a;
    return b + (diff < kMaxTolerance ? jacobian_get(table, diff) : 0.0);
}

// the value of allele a's component at count c: read_allele_likelihood_by_allele_count (:606-660)
__device__ __forceinline__ double component(double m, uint32_t c, const double *__restrict__ log10_k) {
    return c == 1 ? m : m + log10_k[c];
}

}  // namespace

__global__ void __launch_bounds__(GT_THREADS) phmm_genotype_kernel(GenotypeParams p) {
    extern __shared__ double lds[];
    __shared__ uint32_t wave_count[GT_THREADS / 64];
    __shared__ double wave_max[GT_THREADS / 64];

    const uint32_t e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t g_region = p.event_region[e];
    const uint32_t r0 = p.region_read_off[g_region], r1 = p.region_read_off[g_region + 1];
    const uint32_t h0 = p.region_hap_off[g_region], nh = p.region_hap_off[g_region + 1] - h0;
    const double *__restrict__ L = p.likelihoods + p.region_lk_off[g_region];
    const int32_t *__restrict__ map = p.event_hap_allele + p.event_map_off[e];
    const uint32_t A = p.event_allele_off[e + 1] - p.event_allele_off[e];
    const uint32_t G = p.genotype_count[e];
    const int64_t w0 = p.event_start[e], w1 = p.event_end[e];
    const uint32_t ploidy = p.ploidy;
    const double log10_ploidy = p.log10_k[ploidy];

    // the tile: T reads of M[A][T] and terms[G][T] (both <= 1 024 + 1 024 rows: T >= 2)
    uint32_t T = (uint32_t)(GT_LDS_BYTES / (8ull * (A + G)));
    if (T > GT_MAX_TILE) T = GT_MAX_TILE;
    double *M = lds;
    double *terms = lds + (size_t)A * T;

    for (uint32_t s = 0; s < p.n_samples; ++s) {
        double acc[GT_PER_LANE];
#pragma unroll
        for (int k = 0; k < (int)GT_PER_LANE; ++k) acc[k] = 0.0;
        uint32_t n_used = 0;

        for (uint32_t base = r0; base < r1; base += T) {
            // ---- 1. which reads of the tile are used; their order-preserving slots ----
            const uint32_t r = base + t;
            bool use = false;
            if (t < T && r < r1 && p.keep[r] && p.read_sample[r] == s) {
                // Locatable::overlaps (simple_interval.rs:298-307) with the event window as self, the read as other
                const int64_t os = p.read_start[r], oe = p.read_end[r];
                use = (os >= w0 && os <= w1) || (oe >= w0 && oe <= w1) || (w0 >= os && w1 <= oe);
            }
            const uint64_t ballot = __ballot(use);
            const uint32_t before_in_wave = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
            if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
            __syncthreads();
            uint32_t slot = before_in_wave, cnt = 0;
            for (uint32_t w = 0; w < GT_THREADS / 64; ++w) {
                if (w < wave) slot += wave_count[w];
                cnt += wave_count[w];
            }
            if (cnt) {
                for (uint32_t i = t; i < A * cnt; i += GT_THREADS) M[(i / cnt) * T + (i % cnt)] = -INFINITY;
                __syncthreads();
                // marginal_likelihoods: for each haplotype in order, keep the strictly larger value
                if (use) {
                    const double *__restrict__ row = L + (size_t)(r - r0) * nh;
                    for (uint32_t h = 0; h < nh; ++h) {
                        const int32_t a = map[h];
                        if (a < 0) continue;
                        const double v = row[h];
                        double *m = M + (size_t)a * T + slot;
                        if (v > *m) *m = v;
                    }
                }
                __syncthreads();
                // ---- 2. the per-read term of every (read, genotype) pair (:479-580) ----
                for (uint32_t i = t; i < G * cnt; i += GT_THREADS) {
                    const uint32_t g = i / cnt, j = i % cnt;
                    const uint32_t c0 = p.gt_comp_off[g], nc = p.gt_comp_off[g + 1] - c0;
                    double v;
                    if (nc == 1) {
                        const uint32_t ac = p.gt_comp[c0];
                        v = component(M[(ac & 0xffffu) * T + j], ac >> 16, p.log10_k);
                    } else if (nc == 2) {
                        const uint32_t ac0 = p.gt_comp[c0], ac1 = p.gt_comp[c0 + 1];
                        v = approx_sum2(p.jacobian, component(M[(ac0 & 0xffffu) * T + j], ac0 >> 16, p.log10_k),
                                        component(M[(ac1 & 0xffffu) * T + j], ac1 >> 16, p.log10_k));
                    } else {
                        // approximate_log10_sum_log10_vec (math_utils.rs:344-370): from the first maximal component, the
                        // others folded in order, -inf skipped
                        uint32_t imax = 0;
                        double vmax = component(M[(p.gt_comp[c0] & 0xffffu) * T + j], p.gt_comp[c0] >> 16, p.log10_k);
                        for (uint32_t c = 1; c < nc; ++c) {
                            const uint32_t ac = p.gt_comp[c0 + c];
                            const double x = component(M[(ac & 0xffffu) * T + j], ac >> 16, p.log10_k);
                            if (x > vmax) {
                                vmax = x;
                                imax = c;
                            }
                        }
                        v = vmax;
                        for (uint32_t c = 0; c < nc; ++c) {
                            const uint32_t ac = p.gt_comp[c0 + c];
                            const double x = component(M[(ac & 0xffffu) * T + j], ac >> 16, p.log10_k);
                            if (c == imax || x == -INFINITY) continue;
                            const double diff = v - x;
                            if (diff < kMaxTolerance) v += jacobian_get(p.jacobian, diff);
                        }
                    }
                    terms[(size_t)g * T + j] = v;
                }
                __syncthreads();
                // ---- 3. the sum over the reads, in their order (genotype_likelihoods_private, :368-383) ----
#pragma unroll
                for (int k = 0; k < (int)GT_PER_LANE; ++k) {
                    const uint32_t g = t + (uint32_t)k * GT_THREADS;
                    if (g < G) {
                        const double *tg = terms + (size_t)g * T;
                        double a = acc[k];
                        for (uint32_t j = 0; j < cnt; ++j) a += tg[j];
                        acc[k] = a;
                    }
                }
                n_used += cnt;
            }
            __syncthreads();  // (the tile and wave_count are reused)
        }

        // ---- GLs, then the PLs against their maximum ----
        const double denominator = (double)n_used * log10_ploidy;
        const uint64_t out = p.event_out_off[e] + (uint64_t)s * G;
        double m = -INFINITY;
#pragma unroll
        for (int k = 0; k < (int)GT_PER_LANE; ++k) {
            const uint32_t g = t + (uint32_t)k * GT_THREADS;
            if (g < G) {
                acc[k] = acc[k] - denominator;
                p.gl[out + g] = acc[k];
                if (acc[k] > m) m = acc[k];
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double o = __shfl_xor(m, off);
            if (o > m) m = o;
        }
        if (lane == 0) wave_max[wave] = m;
        __syncthreads();
        double adjust = wave_max[0];
        for (uint32_t w = 1; w < GT_THREADS / 64; ++w)
            if (wave_max[w] > adjust) adjust = wave_max[w];
#pragma unroll
        for (int k = 0; k < (int)GT_PER_LANE; ++k) {
            const uint32_t g = t + (uint32_t)k * GT_THREADS;
            if (g < G) p.pl[out + g] = to_pl(acc[k], adjust);
        }
        if (t == 0) p.n_evidence[(size_t)e * p.n_samples + s] = n_used;
        __syncthreads();  // (wave_max is reused by the next sample)
    }
}

hipError_t launch_genotype(const GenotypeParams &p, hipStream_t stream) {
    if (!p.n_events) return hipSuccess;
    hipLaunchKernelGGL(phmm_genotype_kernel, dim3(p.n_events), dim3(GT_THREADS), GT_LDS_BYTES, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
