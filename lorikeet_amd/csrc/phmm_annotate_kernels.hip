// Annotation of called events on the device (phmm_annotate_events, include/phmm.h): for every called event, what the
// reference does with the read likelihoods once calculate_genotypes has returned a call
// (src/haplotype/haplotype_caller_genotyping_engine.rs:330-393, :451-489):
//   AlleleLikelihoods::marginalize onto the alleles of the call (allele_likelihoods.rs:633-740) ->
//   VariantAnnotationEngine::annotate_context (annotator/variant_annotator_engine.rs:32-113) ->
//   the FORMAT fields AD, DP, AF, AC and the INFO fields DP, QD, MQ, BQ (annotator/variant_annotation.rs:93-405).
// One 256-lane workgroup per event.  A lane takes a read (r = r0 + t, r0 + t + T, ...): it tests keep / overlap, marginalizes
// the read's row into its own column of M[C][T] in LDS (strict >, haplotypes in order, from -inf: the reference's loop), runs
// search_best_allele over the column and counts the read with LDS integer atomics -- AD per (sample, best allele), and for the
// reads with mapq != 0 a 256-bin histogram of MQ and of BQ per best allele.  Counts do not depend on the order in which lanes or
// waves arrive, and the upper median is a prefix walk over the bins: exact, no sort.  What does not fit in LDS at once is done
// in passes over the reads: pass k counts AD for the k-th chunk of samples and the histograms of the k-th group of ANN_GROUP
// call alleles (one pass for up to 8 call alleles and 2 048 / C samples).
// The floating-point work is comparisons, one subtraction per read and one division per output (built with
// -ffp-contract=off), so the results are the reference's bits.
#include <algorithm>
#include <cfloat>

#include "../../include/phmm.h"
#include "phmm_annotate_internal.hpp"

namespace phmm {
namespace {

// AssemblyBasedCallerUtils::reference_tiebreaking_priority (assembly_based_caller_utils.rs:197-199); allele 0 of a call is the reference
__device__ __forceinline__ int priority(uint32_t a) { return a == 0 ? 1 : 0; }

// AlleleLikelihoods::search_best_allele with can_be_reference = true and priorities present (allele_likelihoods.rs:457-554),
// BestAllele::new and is_informative (:1142-1165), over the lane's column col[a * T], a < C (C >= 1)
__device__ __forceinline__ bool search_best_allele(const double *col, uint32_t T, uint32_t C, uint32_t *best_out) {
    uint32_t best = 0, second = 0;
    double best_lk = col[0], second_lk = -INFINITY;
    for (uint32_t a = 1; a < C; ++a) {
        const double v = col[(size_t)a * T];
        if (v > best_lk) {
            second = best;
            best = a;
            second_lk = best_lk;
            best_lk = v;
        } else if (v > second_lk) {
            second = a;
            second_lk = v;
        }
    }
    if (best_lk - second_lk < ANN_INFORMATIVE) {
        // ties: among everything within the threshold of the best likelihood, the highest priority wins (:512-536)
        int best_pri = priority(best), second_pri = priority(second);
        for (uint32_t a = 0; a < C; ++a) {
            const double v = col[(size_t)a * T];
            if (a == best || best_lk - v > ANN_INFORMATIVE) continue;
            const int pri = priority(a);
            if (pri > best_pri) {
                second = best;
                best = a;
                second_pri = best_pri;
                best_pri = pri;
            } else if (pri > second_pri) {
                second = a;
                second_pri = pri;
            }
        }
    }
    best_lk = col[(size_t)best * T];
    second_lk = second != best ? col[(size_t)second * T] : -INFINITY;
    const double d = best_lk - second_lk;
    const double confidence = fabs(d) < DBL_EPSILON ? 0.0 : d;
    *best_out = best;
    return confidence > ANN_INFORMATIVE;
}

// ReadUtils::get_read_base_quality_at_reference_coordinate (reads/read_utils.rs:103-173): -1 = None.  The walk starts at the
// soft start; soft clips advance the reference position; inside an element that consumes no read bases there is no quality.
__device__ __forceinline__ int base_quality_at(const AnnotateParams &p, uint32_t r, int64_t pos) {
    if (pos < p.read_start[r] || p.read_end[r] < pos) return -1;
    int64_t last_ref = p.read_soft_start[r];
    if (pos < last_ref) return -1;
    uint64_t last_read = 0;
    for (uint32_t i = p.cigar_off[r]; i < p.cigar_off[r + 1]; ++i) {
        const uint32_t el = p.cigar[i], len = el >> 4, op = el & 15u;
        const bool on_read = op == 0 || op == 1 || op == 4 || op == 7 || op == 8;  // M I S = X (cigar_utils.rs:105-115)
        const bool on_ref = op == 0 || op == 2 || op == 3 || op == 7 || op == 8 || op == 4;  // M D N = X (:117-127), or a soft clip
        const uint64_t first_read = last_read;
        const int64_t first_ref = last_ref;
        if (on_read) last_read += len;
        if (on_ref) last_ref += len;
        if (first_ref <= pos && pos < last_ref) {
            if (!on_read) return -1;
            const uint64_t at = first_read + (uint64_t)(pos - first_ref);
            const uint32_t b0 = p.read_off[r];
            if (at >= (uint64_t)(p.read_off[r + 1] - b0)) return -1;  // (a CIGAR longer than its read: the reference panics)
            return p.base_q[b0 + at];
        }
    }
    return -1;
}

// MathUtils::median (utils/math_utils.rs:41-45): the element at index len / 2 of the sorted values; 30 when there are none
// (variant_annotation.rs:223-233).  One whole wave per histogram: a lane sums four bins, an inclusive scan over the wave gives
// the count up to each lane, the first lane whose count passes len / 2 walks its four bins.
__device__ __forceinline__ uint8_t upper_median(const uint32_t *bins, uint32_t lane) {
    const uint32_t b0 = bins[4 * lane], b1 = bins[4 * lane + 1], b2 = bins[4 * lane + 2], b3 = bins[4 * lane + 3];
    const uint32_t own = b0 + b1 + b2 + b3;
    uint32_t upto = own;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(upto, off);
        if (lane >= off) upto += o;
    }
    const uint32_t n = __shfl(upto, 63);
    if (!n) return 30;
    const uint32_t mid = n / 2;
    const int first = __ffsll((unsigned long long)__ballot(upto > mid)) - 1;  // (lane 63 holds n > mid: there is one)
    uint32_t seen = upto - own, v = 4 * lane;
    if ((seen += b0) <= mid) {
        ++v;
        if ((seen += b1) <= mid) {
            ++v;
            if ((seen += b2) <= mid) ++v;
        }
    }
    return (uint8_t)__shfl(v, first);
}

}  // namespace

__global__ void __launch_bounds__(ANN_THREADS) phmm_annotate_kernel(AnnotateParams p) {
    extern __shared__ double M[];
    __shared__ uint32_t hist[2][ANN_GROUP][256];  // [MQ | BQ][call allele of the group][value]
    __shared__ int32_t ad[ANN_AD_SLOTS];          // [sample of the chunk][call allele]
    __shared__ int32_t n_used[ANN_MAX_CHUNK];     // the reads used per sample of the chunk
    __shared__ int32_t depth[3];                  // get_depth's depth and AD_restrict_depth; the sum of DP

    const uint32_t e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t S = p.n_samples;
    const uint32_t co = p.call_off[e], C = p.call_off[e + 1] - co;
    const size_t es = (size_t)e * S;
    if (!C) {  // not annotated: everything 0
        for (uint32_t s = t; s < S; s += ANN_THREADS) {
            p.dp[es + s] = 0;
            p.ac[es + s] = 0;
        }
        if (t == 0) {
            p.info_dp[e] = 0;
            p.qd_depth[e] = 0;
            p.qd[e] = 0.0;
            p.flags[e] = 0;
        }
        return;
    }
    const uint32_t g_region = p.event_region[e];
    const uint32_t r0 = p.region_read_off[g_region], r1 = p.region_read_off[g_region + 1];
    const uint32_t nh = p.region_hap_off[g_region + 1] - p.region_hap_off[g_region];
    const double *__restrict__ L = p.likelihoods + p.region_lk_off[g_region];
    const int32_t *__restrict__ map = p.event_hap_call + p.event_map_off[e];
    const int64_t w0 = p.event_start[e], w1 = p.event_end[e];
    const bool no_ad = C <= 1;  // DepthPerAlleleBySample returns before it sets AD (variant_annotation.rs:250-252)
    const bool with_bq = p.base_q != nullptr;
    const int64_t pos = with_bq ? p.event_pos[e] : 0;

    uint32_t T = (uint32_t)(ANN_LDS_BYTES / (8ull * C));
    if (T > ANN_MAX_TILE) T = ANN_MAX_TILE;
    uint32_t chunk = ANN_AD_SLOTS / C;
    if (chunk > ANN_MAX_CHUNK) chunk = ANN_MAX_CHUNK;
    const uint32_t n_chunks = (S + chunk - 1) / chunk, n_groups = (C + ANN_GROUP - 1) / ANN_GROUP;
    const uint32_t n_pass = n_chunks > n_groups ? n_chunks : n_groups;
    double *col = M + t;

    if (t < 3) depth[t] = 0;
    for (uint32_t k = 0; k < n_pass; ++k) {
        const uint32_t s0 = k < n_chunks ? k * chunk : S, s1 = s0 + chunk < S ? s0 + chunk : S;
        const uint32_t c0 = k < n_groups ? k * ANN_GROUP : C, c1 = c0 + ANN_GROUP < C ? c0 + ANN_GROUP : C;
        for (uint32_t i = t; i < (c1 - c0) * 256; i += ANN_THREADS) (&hist[0][0][0])[i] = (&hist[1][0][0])[i] = 0;
        for (uint32_t i = t; i < (s1 - s0) * C; i += ANN_THREADS) ad[i] = 0;
        for (uint32_t i = t; i < s1 - s0; i += ANN_THREADS) n_used[i] = 0;
        __syncthreads();

        if (t < T) {
            for (uint64_t r64 = (uint64_t)r0 + t; r64 < r1; r64 += T) {
                const uint32_t r = (uint32_t)r64;
                if (!p.keep[r]) continue;
                const uint32_t s = p.read_sample[r];
                const bool count_ad = s >= s0 && s < s1;
                if (!count_ad && c0 == c1) continue;
                // Locatable::overlaps (simple_interval.rs:298-307) with the event window as self, the read as other
                const int64_t os = p.read_start[r], oe = p.read_end[r];
                if (!((os >= w0 && os <= w1) || (oe >= w0 && oe <= w1) || (w0 >= os && w1 <= oe))) continue;
                // marginal_likelihoods onto the call's alleles: for each haplotype in order, keep the strictly larger value
                for (uint32_t a = 0; a < C; ++a) col[(size_t)a * T] = -INFINITY;
                const double *__restrict__ row = L + (size_t)(r - r0) * nh;
                for (uint32_t h = 0; h < nh; ++h) {
                    const int32_t a = map[h];
                    if (a < 0) continue;
                    const double v = row[h];
                    double *m = col + (size_t)a * T;
                    if (v > *m) *m = v;
                }
                uint32_t best;
                const bool informative = search_best_allele(col, T, C, &best);
                if (count_ad) {
                    atomicAdd(&n_used[s - s0], 1);
                    if (informative && !no_ad) atomicAdd(&ad[(s - s0) * C + best], 1);  // (:265-272)
                }
                // MQ / BQ: the informative reads of every sample with mapq != 0 (is_usable_read), by best allele (:188-221)
                if (informative && best >= c0 && best < c1) {
                    const uint8_t q = p.mapq[r];
                    if (q != 0) {
                        atomicAdd(&hist[0][best - c0][q], 1u);
                        if (with_bq) {
                            const int b = base_quality_at(p, r, pos);
                            if (b >= 0) atomicAdd(&hist[1][best - c0][b], 1u);
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- the samples of the chunk: AD, DP, AF, AC and their share of get_depth (:360-405) ----
        for (uint32_t i = t; i < s1 - s0; i += ANN_THREADS) {
            const uint32_t s = s0 + i;
            const int32_t *a = ad + (size_t)i * C;
            int32_t total = 0;
            uint32_t n_pos = 0;
            for (uint32_t c = 0; c < C; ++c) {
                total += a[c];
                n_pos += a[c] > 0;
            }
            const size_t out = (size_t)S * co + (size_t)s * C;
            const double sum = (double)total;  // normalize_sum_to_one's sum of the counts (math_utils.rs:402-415): exact
            for (uint32_t c = 0; c < C; ++c) {
                p.ad[out + c] = a[c];
                p.af[out + c] = no_ad ? 0.0 : (double)a[c] / sum;
            }
            p.dp[es + s] = total;
            p.ac[es + s] = n_pos;
            atomicAdd(&depth[2], total);
            if (p.sample_called && !p.sample_called[es + s]) continue;  // a no-call is skipped (:367-377)
            if (!no_ad && total != 0) {
                if (total - a[0] > 0) atomicAdd(&depth[1], total);
                atomicAdd(&depth[0], total);
            } else {
                atomicAdd(&depth[0], n_used[i] + (p.n_filtered ? (int32_t)p.n_filtered[es + s] : 0));  // sample_evidence_count (:393-394)
            }
        }
        // ---- the call alleles of the group: the upper medians, a wave per histogram ----
        for (uint32_t i = wave; i < (with_bq ? 2u : 1u) * (c1 - c0); i += ANN_THREADS / 64) {
            const uint32_t kind = i / (c1 - c0), c = i % (c1 - c0);
            const uint8_t m = upper_median(hist[kind][c], lane);
            if (lane == 0) (kind == 0 ? p.mq : p.bq)[co + c0 + c] = m;
        }
        __syncthreads();  // (the counters are cleared by the next pass)
    }

    if (t == 0) {
        // QualByDepth (:295-328)
        const int32_t d = depth[1] > 0 ? depth[1] : depth[0];
        const double err = p.log10_p_error[e];
        const bool has_error = err == err && fabs(err - 1.0) > DBL_EPSILON;  // has_log10_p_error (variant_context.rs:230-232); NaN: none
        uint32_t flags = no_ad ? PHMM_ANN_NO_AD : 0u;
        double qd = 0.0;
        if (!has_error || S == 0 || d == 0) {
            flags |= PHMM_ANN_NO_QD;
        } else {
            const double qual = -10.0 * err;
            qd = qual / (double)d;
            if (!(qd < ANN_MAX_QD)) flags |= PHMM_ANN_QD_JITTER;  // fix_too_high_qd (:416-424) draws from a thread RNG: the caller's
        }
        p.info_dp[e] = depth[2];
        p.qd_depth[e] = d;
        p.qd[e] = qd;
        p.flags[e] = flags;
    }
}

hipError_t launch_annotate(const AnnotateParams &p, uint32_t max_call_alleles, hipStream_t stream) {
    if (!p.n_events) return hipSuccess;
    // an event's tile is C x T doubles, T = min(ANN_MAX_TILE, ANN_LDS_BYTES / 8 C): at most min(ANN_MAX_TILE x C, ANN_LDS_BYTES / 8),
    // which grows with C -- the batch's largest call bounds every event's
    const size_t C = max_call_alleles ? max_call_alleles : 1;
    const size_t lds = std::min<size_t>(8 * ANN_MAX_TILE * C, ANN_LDS_BYTES);
    hipLaunchKernelGGL(phmm_annotate_kernel, dim3(p.n_events), dim3(ANN_THREADS), lds, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
