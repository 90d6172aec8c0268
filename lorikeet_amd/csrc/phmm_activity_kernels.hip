// The activity profile on the device (phmm_activity_profile, include/phmm.h), the reference's stage in front of assembly:
//   activity_read_kernel      HaplotypeCallerEngine::parse_record -> alignment_context_creation up to the point where a pileup
//                             entry touches its position (src/haplotype/haplotype_caller_engine.rs:754-899, :1464-1722): one
//                             wave per read writes the read's slots (counted, is_alt, quality, adds soft clips), the table
//                             "position -> first slot" and count_high_quality_soft_clips
//   activity_site_kernel      the sums of update_heterozygous_likelihood (:1724-1749), the depths, the soft-clip RunningAverage
//                             (math_utils.rs:434-477) and update_ref_vs_any_results (:738-752), then gls_to_pls: one lane per
//                             (window, position), samples and reads in order
//   activity_events_kernel    the uniform event list phmm_af_kernel runs on: reference + one symbolic alt per position
//   activity_prob_kernel      is_active_prob (:1080-1085) and how often process_state re-emits a position's band
//                             (activity_profile.rs:308-341)
//   activity_bandpass_kernel  BandPassActivityProfile::add as a gather (band_pass_activity_profile.rs:210-280,
//                             activity_profile.rs:263-289): one lane per list entry, sources ascending
//   activity_length_kernel    the length of each profile's state list
// Floating point: f64 and f32 additions, one f64 subtraction, multiplication and division, in the reference's order; compile
// with -ffp-contract=off.  Everything transcendental comes from the host as tables.
#include "phmm_activity_internal.hpp"
#include "phmm_genotype_internal.hpp"

#include "../../include/phmm.h"

namespace phmm {
namespace {

constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4, OP_EQ = 7, OP_X = 8;

__device__ __forceinline__ bool consumes_read(uint32_t op) { return op == OP_M || op == OP_I || op == OP_S || op == OP_EQ || op == OP_X; }
__device__ __forceinline__ uint8_t upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }

// check_position_against_cigar (:1654-1687)
__device__ __forceinline__ bool check_against(uint32_t op, bool check_indels) {
    return op == OP_S || ((op == OP_I || op == OP_D) && check_indels);
}

// next_to_soft_clip_or_indel (:1596-1652), loop for loop: two cursors, the one-based comparison, the `else if`, the early break
__device__ bool next_to_soft_clip_or_indel(const uint32_t *__restrict__ cigar, uint32_t n_cigar, int32_t qpos, bool check_indels) {
    int32_t read_cursor = 0, end_of_cigar_read_cursor = 0;
    bool next_to_soft_clip = false;
    const int32_t qpos_to_cigar_cursor = qpos + 1;
    for (uint32_t c = 0; c < n_cigar; ++c) {
        const uint32_t op = cigar[c] & 15u;
        const int32_t len = (int32_t)(cigar[c] >> 4);
        if (consumes_read(op)) end_of_cigar_read_cursor = read_cursor + len;
        if (qpos_to_cigar_cursor == read_cursor) next_to_soft_clip = check_against(op, check_indels);
        else if (qpos_to_cigar_cursor - 1 == end_of_cigar_read_cursor) next_to_soft_clip = check_against(op, check_indels);
        const bool past_query_pos = read_cursor >= qpos;
        if (past_query_pos || next_to_soft_clip) break;
        if (consumes_read(op)) read_cursor += len;
    }
    return next_to_soft_clip;
}

// alignment_context_creation for an entry with a read base (:1480-1520): the slot's code
__device__ uint16_t base_slot(const ActivityParams &p, const uint32_t *__restrict__ cigar, uint32_t n_cigar, const uint8_t *__restrict__ bases,
                              const uint8_t *__restrict__ quals, uint32_t read_len, uint32_t qpos, uint8_t ref_base) {
    if (qpos >= read_len) return 0;  // (never: the host rejected CIGARs that consume more than the read has)
    const uint32_t q = quals[qpos];
    uint16_t code = (uint16_t)(q << 8);
    if (q >= p.bq) {  // is_alt is never evaluated for an uncounted base
        code |= ACT_SLOT_COUNTED;
        const bool alt = upper(bases[qpos]) != upper(ref_base) || next_to_soft_clip_or_indel(cigar, n_cigar, (int32_t)qpos, true);
        if (alt) {
            code |= ACT_SLOT_ALT;
            if (next_to_soft_clip_or_indel(cigar, n_cigar, (int32_t)qpos, false)) code |= ACT_SLOT_SOFTCLIPS;
        }
    }
    return code;
}

__global__ void __launch_bounds__(ACT_THREADS) activity_read_kernel(ActivityParams p) {
    const uint32_t r = blockIdx.x * (ACT_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= p.n_reads) return;
    const uint32_t span = p.read_span[r], w = p.read_window[r];
    if (!span || p.win_status[w] < 0) return;
    const uint32_t *__restrict__ cigar = p.cigar + p.cigar_off[r];
    const uint32_t n_cigar = p.cigar_off[r + 1] - p.cigar_off[r];
    const uint8_t *__restrict__ bases = p.read_bases + p.read_off[r];
    const uint8_t *__restrict__ quals = p.read_quals + p.read_off[r];
    const int64_t bound_start = p.win_start[w], bound_end = p.win_end[w], lo = p.read_lo[r];
    const uint8_t *__restrict__ ref = p.ref_bases + p.ref_off[w];
    uint16_t *__restrict__ slots = p.ws_slot + p.slot_off[r];
    uint32_t *__restrict__ tab = p.ws_tab + p.tab_off[r];
    const uint32_t slot_cap = (uint32_t)(p.slot_off[r + 1] - p.slot_off[r]), read_len = p.read_off[r + 1] - p.read_off[r];

    // count_high_quality_soft_clips (:1689-1722): one number per read
    {
        uint32_t align_pos = 0, n_hq = 0;
        for (uint32_t c = 0; c < n_cigar; ++c) {
            const uint32_t op = cigar[c] & 15u, len = cigar[c] >> 4;
            if (op == OP_S)
                for (uint32_t j = 0; j < len; j += 64) n_hq += (uint32_t)__popcll(__ballot(j + lane < len && align_pos + j + lane < read_len && quals[align_pos + j + lane] > ACT_SOFTCLIP_QUAL));
            if (consumes_read(op)) align_pos += len;
        }
        if (lane == 0) p.read_softclips[r] = (double)n_hq;
    }

    int64_t pos = p.read_pos[r], last_pos = INT64_MIN;
    uint32_t read_cursor = 0, cig_index = 0, n_slots = 0;
    for (uint32_t c = 0; c < n_cigar; ++c) {
        const uint32_t op = cigar[c] & 15u, len = cigar[c] >> 4;
        if (op == OP_D || op == OP_M || op == OP_EQ || op == OP_X) {
            // bases before bound_start advance the cursors without an entry; the first one at or past bound_end ends the element
            const int64_t a = bound_start - pos, b = bound_end - pos;
            const uint32_t j0 = a <= 0 ? 0u : a >= (int64_t)len ? len : (uint32_t)a;
            const uint32_t j1 = b <= 0 ? 0u : b >= (int64_t)len ? len : (uint32_t)b;
            const bool joins = j1 > j0 && last_pos == pos + j0;  // an I element put its slot at this position already
            uint16_t del_code = 0;
            if (op == OP_D) {
                // next_to_soft_clip of a deletion (:1539-1545) looks at the elements around cig_index, which lags after an
                // I element before bound_start
                const uint32_t before = cig_index ? cig_index - 1 : 0, after = cig_index + 1 < n_cigar - 1 ? cig_index + 1 : n_cigar - 1;
                const bool sc = (cigar[before] & 15u) == OP_S || (cigar[after] & 15u) == OP_S || (cigar[cig_index] & 15u) == OP_S;
                del_code = (uint16_t)((ACT_DELETION_QUAL << 8) | ACT_SLOT_COUNTED | ACT_SLOT_ALT | (sc ? ACT_SLOT_SOFTCLIPS : 0));
            }
            for (uint32_t j = j0 + lane; j < j1; j += 64) {
                const uint32_t s = n_slots + (j - j0);
                if (s >= slot_cap) break;  // (never: the host counted the slots)
                const int64_t at = pos + j;
                slots[s] = op == OP_D ? del_code : base_slot(p, cigar, n_cigar, bases, quals, read_len, read_cursor + j, ref[at - bound_start]);
                if (!(joins && j == j0) && (uint64_t)(at - lo) < span) tab[at - lo] = s;
            }
            if (j1 > j0) {
                n_slots += j1 - j0;
                last_pos = pos + j1 - 1;
            }
            if (op != OP_D) read_cursor += j1;
            pos += j1;
        } else if (op == OP_I) {
            if (pos < bound_start) {
                read_cursor += len;
                continue;  // as the reference: cig_index is not advanced
            } else if (pos >= bound_end) {
                break;
            }
            if (lane == 0 && n_slots < slot_cap) {
                slots[n_slots] = base_slot(p, cigar, n_cigar, bases, quals, read_len, read_cursor, ref[pos - bound_start]);
                if (last_pos != pos && (uint64_t)(pos - lo) < span) tab[pos - lo] = n_slots;
            }
            last_pos = pos;
            n_slots += 1;
            read_cursor += len;
        } else if (op == OP_S) {
            read_cursor += len;
        }
        cig_index += 1;
    }
    // positions after the last slot (the place of a trailing insertion that is not there), and the end of the table
    const uint32_t first_free = last_pos == INT64_MIN ? 0u : (uint32_t)(last_pos - lo) + 1;
    for (uint32_t k = first_free + lane; k <= span; k += 64) tab[k] = n_slots;
}

__device__ __forceinline__ uint32_t window_of(const uint32_t *__restrict__ pos_off, uint32_t n_windows, uint32_t gpos) {
    uint32_t a = 0, b = n_windows;  // the last w with pos_off[w] <= gpos
    while (b - a > 1) {
        const uint32_t m = (a + b) >> 1;
        if (pos_off[m] <= gpos) a = m;
        else b = m;
    }
    return a;
}

template <int CH>
__global__ void __launch_bounds__(ACT_THREADS) activity_site_kernel(ActivityParams p) {
    const uint32_t gpos = blockIdx.x * ACT_THREADS + threadIdx.x;
    if (gpos >= p.n_pos) return;
    const uint32_t w = window_of(p.pos_off, p.n_windows, gpos), G = p.G, S = p.n_samples;
    const int64_t pos = p.win_start[w] + (int64_t)(gpos - p.pos_off[w]);
    const bool dead = p.win_status[w] < 0;
    double mean = 0.0;
    uint32_t n_obs = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t grp = w * S + s;
        uint32_t r0 = p.group_read_off[grp], r1 = dead ? r0 : p.group_read_off[grp + 1];
        // the reads that can cover the position: from the first whose running maximum end exceeds it to the first that starts
        // after it
        uint32_t lo = r0, hi = r1;
        {
            uint32_t a = r0, b = r1;
            while (a < b) {
                const uint32_t m = (a + b) >> 1;
                if (p.read_pmax_end[m] > pos) b = m;
                else a = m + 1;
            }
            lo = a;
            b = r1;
            while (a < b) {
                const uint32_t m = (a + b) >> 1;
                if (p.read_lo[m] > pos) b = m;
                else a = m + 1;
            }
            hi = a;
        }
        uint32_t read_counts = 0, ref_depth = 0, non_ref_depth = 0;
        const size_t out = (size_t)gpos * S + s;
        double *__restrict__ gl = p.gl + out * G;
        for (uint32_t g0 = 0; g0 < G; g0 += CH) {
            double acc[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] = 0.0;
            for (uint32_t r = lo; r < hi; ++r) {
                const int64_t k = pos - p.read_lo[r];
                if (k >= (int64_t)p.read_span[r]) continue;
                const uint32_t *__restrict__ tab = p.ws_tab + p.tab_off[r] + k;
                const uint16_t *__restrict__ slots = p.ws_slot + p.slot_off[r];
                const uint32_t n_read_slots = (uint32_t)(p.slot_off[r + 1] - p.slot_off[r]);
                const uint32_t s1 = tab[1] < n_read_slots ? tab[1] : n_read_slots;  // (the table never points past the read's slots)
                for (uint32_t sl = tab[0]; sl < s1; ++sl) {
                    const uint32_t code = slots[sl];
                    if (!(code & ACT_SLOT_COUNTED)) continue;
                    const uint32_t alt = (code >> 1) & 1u;
                    const double *__restrict__ t = p.term + ((size_t)(alt * 256u + (code >> 8)) * G + g0);
#pragma unroll
                    for (int c = 0; c < CH; ++c)
                        if (g0 + c < G) acc[c] += t[c];
                    if (g0 == 0) {
                        read_counts += 1;
                        non_ref_depth += alt;
                        ref_depth += 1u - alt;
                        if (code & ACT_SLOT_SOFTCLIPS) {  // RunningAverage::add
                            n_obs += 1;
                            mean += (p.read_softclips[r] - mean) / (double)n_obs;
                        }
                    }
                }
            }
            const double denominator = (double)read_counts * p.log10_ploidy;  // update_ref_vs_any_results
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (g0 + c < G) gl[g0 + c] = acc[c] - denominator;
        }
        p.read_counts[out] = read_counts;
        p.ref_depth[out] = ref_depth;
        p.non_ref_depth[out] = non_ref_depth;
        double adjust = -INFINITY;
        for (uint32_t g = 0; g < G; ++g) {
            const double x = gl[g];
            if (!(x < adjust)) adjust = x;
        }
        int32_t *__restrict__ pl = p.pl + out * G;
        for (uint32_t g = 0; g < G; ++g) pl[g] = to_pl(gl[g], adjust);
    }
    p.softclip_mean[gpos] = mean;
    p.softclip_count[gpos] = n_obs;
}

__global__ void __launch_bounds__(ACT_THREADS) activity_events_kernel(ActivityParams p, uint32_t *work, uint32_t *allele_off, uint32_t *genotype_count,
                                                                       int32_t *span_del, uint64_t *pl_off, double *prior, uint8_t *kind) {
    const uint32_t i = blockIdx.x * ACT_THREADS + threadIdx.x;
    if (i > p.n_pos) return;
    allele_off[i] = 2 * i;
    if (i == p.n_pos) return;
    work[i] = i;
    genotype_count[i] = p.G;
    span_del[i] = -1;
    pl_off[i] = (uint64_t)i * p.n_samples * p.G;
    prior[2 * i] = p.ref_pseudo;
    prior[2 * i + 1] = p.indel_pseudo;  // a symbolic allele of length 0 is not of the reference's length: the indel class
    kind[2 * i] = kind[2 * i + 1] = 0;  // plain alleles
}

__global__ void __launch_bounds__(ACT_THREADS) activity_prob_kernel(ActivityParams p) {
    const uint32_t gpos = blockIdx.x * ACT_THREADS + threadIdx.x;
    if (gpos >= p.n_pos) return;
    const uint32_t w = window_of(p.pos_off, p.n_windows, gpos);
    if (p.win_status[w] < 0) {
        p.qual[gpos] = 0.0;
        p.af_flags[gpos] = 0;
        p.is_active_prob[gpos] = 0.0f;
        p.mult[gpos] = 1;
        return;
    }
    // vc.get_phred_scaled_qual() as u8: saturating, NaN -> 0
    const double q = p.qual[gpos];
    const uint32_t qi = !(q > 0.0) ? 0u : q >= 255.0 ? 255u : (uint32_t)q;
    p.is_active_prob[gpos] = (p.af_flags[gpos] & PHMM_AF_CALLED) ? p.prob_of_qual[qi] : 0.0f;
    // ActivityProfileDataType::new and ActivityProfile::process_state: the states a soft-clip state turns into
    const float clips = (float)p.softclip_mean[gpos];
    uint32_t mult = 1;
    if (clips >= ACT_SOFTCLIP_MEAN) {
        const int64_t K = (int64_t)(clips < p.max_prob_propagation ? clips : p.max_prob_propagation);
        const int64_t s = p.win_start[w] + (int64_t)(gpos - p.pos_off[w]), L = p.contig_len[w];
        const int64_t a = s - K < 0 ? 0 : s - K, b = s + K > L ? L : s + K;
        mult = b >= a ? (uint32_t)(b - a + 1) : 0u;
    }
    p.mult[gpos] = mult;
}

__global__ void __launch_bounds__(ACT_THREADS) activity_bandpass_kernel(ActivityParams p) {
    const uint32_t k = blockIdx.x, j = blockIdx.y * ACT_THREADS + threadIdx.x;
    const uint32_t n = p.prof_n[k], w = p.prof_window[k], g0 = p.prof_pos[k];
    if (j >= n + p.max_filter) return;
    float *__restrict__ out = p.profile_prob + ((size_t)g0 + (size_t)k * p.max_filter);
    const int64_t F = p.F, start = p.win_start[w] + (int64_t)(g0 - p.pos_off[w]);
    float acc = 0.0f;
    if (p.win_status[w] >= 0 && start + (int64_t)j <= p.contig_len[w]) {
        const int64_t a = (int64_t)j - F < 0 ? 0 : (int64_t)j - F, b = (int64_t)j + F >= (int64_t)n ? (int64_t)n - 1 : (int64_t)j + F;
        for (int64_t s = a; s <= b; ++s) {
            const float prob = p.is_active_prob[g0 + s];
            if (!(prob > 0.0f)) continue;
            const float term = prob * p.taps[(int64_t)j - s + F];
            for (uint32_t m = p.mult[g0 + s]; m; --m) acc += term;
        }
    }
    out[j] = acc;
}

__global__ void __launch_bounds__(ACT_THREADS) activity_length_kernel(ActivityParams p) {
    __shared__ uint32_t best[ACT_THREADS];
    const uint32_t k = blockIdx.x, n = p.prof_n[k], w = p.prof_window[k], g0 = p.prof_pos[k];
    const int64_t start = p.win_start[w] + (int64_t)(g0 - p.pos_off[w]), L = p.contig_len[w];
    uint32_t len = 0;
    if (p.win_status[w] >= 0)
        for (uint32_t s = threadIdx.x; s < n; s += ACT_THREADS) {
            int64_t last = s;  // a state without probability is appended where it stands
            if (p.is_active_prob[g0 + s] > 0.0f) {
                last = (int64_t)s + p.F;
                if (start + last > L) last = L - start;
            }
            if (last + 1 > (int64_t)len) len = (uint32_t)(last + 1);
        }
    best[threadIdx.x] = len;
    __syncthreads();
    for (uint32_t h = ACT_THREADS / 2; h; h >>= 1) {
        if (threadIdx.x < h && best[threadIdx.x + h] > best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.profile_len[k] = best[0];
}

}  // namespace

hipError_t launch_activity_pileup(const ActivityParams &p, hipStream_t stream) {
    if (p.n_reads) hipLaunchKernelGGL(activity_read_kernel, dim3((p.n_reads + ACT_THREADS / 64 - 1) / (ACT_THREADS / 64)), dim3(ACT_THREADS), 0, stream, p);
    if (p.n_pos) {
        const dim3 grid((p.n_pos + ACT_THREADS - 1) / ACT_THREADS);
        if (p.G <= 4) hipLaunchKernelGGL(activity_site_kernel<4>, grid, dim3(ACT_THREADS), 0, stream, p);
        else hipLaunchKernelGGL(activity_site_kernel<8>, grid, dim3(ACT_THREADS), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_activity_events(const ActivityParams &p, uint32_t *work, uint32_t *allele_off, uint32_t *genotype_count,
                                  int32_t *span_del, uint64_t *pl_off, double *prior, uint8_t *kind, hipStream_t stream) {
    hipLaunchKernelGGL(activity_events_kernel, dim3(p.n_pos / ACT_THREADS + 1), dim3(ACT_THREADS), 0, stream, p, work, allele_off, genotype_count,
                       span_del, pl_off, prior, kind);
    return hipGetLastError();
}

hipError_t launch_activity_bandpass(const ActivityParams &p, hipStream_t stream) {
    if (!p.n_pos) return hipSuccess;
    hipLaunchKernelGGL(activity_prob_kernel, dim3((p.n_pos + ACT_THREADS - 1) / ACT_THREADS), dim3(ACT_THREADS), 0, stream, p);
    if (!p.n_profiles) return hipGetLastError();
    hipLaunchKernelGGL(activity_length_kernel, dim3(p.n_profiles), dim3(ACT_THREADS), 0, stream, p);
    // grid.y: the longest profile's list (a shorter one's spare workgroups return at once)
    hipLaunchKernelGGL(activity_bandpass_kernel, dim3(p.n_profiles, (p.max_prof_n + p.max_filter + ACT_THREADS - 1) / ACT_THREADS), dim3(ACT_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
