// phmm_phase_calls (include/phmm.h): the tail of the reference's assign_genotype_likelihoods -- reverse_trim_alleles as
// make_annotated_call applies it (haplotype_caller_genotyping_engine.rs:451-489, variant_context_utils.rs:956-1108,
// alignment_utils.rs:585-675), the called haplotypes (:394-405) and phase_calls (assembly_based_caller_utils.rs:975-1348).
// Integers and bytes only.  Five kernels on one stream, each a stage the next one needs finished for every event:
//   phase_trim_kernel     a lane per event: rev_trim and the call's end
//   phase_called_kernel   a wave per event, 64 haplotypes a pass: the called predicate OR-ed into the region's bitset
//   phase_match_kernel    a wave per event, 64 haplotypes a pass: S_e = the called haplotypes whose event map holds the call's
//                         one site-specific alt at the call's start; a ballot is one word of the bitset
//   phase_link_kernel     a wave per region: construct_phase_set_mapping, i serial, j 64 a pass
//   phase_apply_kernel    a lane per (event, sample): leader, phase set, the phased GT
// The one atomic is the OR of phase_called_kernel, whose result does not depend on its order; every other output element has
// one writer, so a call's bytes do not depend on scheduling or on the batch.
#include "phmm_phase_internal.hpp"

namespace phmm {

namespace {

struct CallAlleles {   // the alleles of event e's call
    uint32_t a0, A, c0, C;
};

__device__ inline CallAlleles call_of(const PhaseParams &p, uint32_t e) {
    CallAlleles c;
    c.a0 = p.event_allele_off[e];
    c.A = p.event_allele_off[e + 1] - c.a0;
    c.c0 = p.call_allele_off[e];
    c.C = p.call_allele_off[e + 1] - c.c0;
    return c;
}

// trim_alleles(vc, false, true) on the call's alleles: the bases that leave the end of every allele that is not symbolic.
// normalize_alleles moves every range's start together and every range's end together, so the ranges are [s, len_n - t).
__device__ uint32_t reverse_trim(const PhaseParams &p, const CallAlleles &c) {
    if (c.C <= 1) return 0;                                            // variant_context_utils.rs:961
    uint32_t min_len = 0xffffffffu, n_seq = 0;
    for (uint32_t k = 0; k < c.C; ++k) {
        const uint32_t a = c.a0 + p.call_allele[c.c0 + k];
        if (p.allele_kind[a] == PH_KIND_NON_REF) continue;             // symbolic: left out of the sequences (:970-981)
        const uint32_t len = p.allele_length[a];
        if (len == 1) return 0;                                        // :962-967; '*' is such an allele
        min_len = min(min_len, len);
        ++n_seq;
    }
    if (!n_seq) return 0;                                              // (the host refuses a symbolic reference allele)
    const uint32_t a_first = c.a0;                                     // sequences[0]: the reference, entry 0 of every call
    const uint8_t *first = p.allele_bases + p.allele_bases_off[a_first];
    const uint32_t first_len = p.allele_length[a_first];
    // is the byte at `at` from the start (from_end == false) or `at` before the end the same in every sequence
    const auto same = [&](bool from_end, uint32_t at) {
        const uint8_t b = from_end ? first[first_len - at] : first[at];
        for (uint32_t k = 1; k < c.C; ++k) {
            const uint32_t a = c.a0 + p.call_allele[c.c0 + k];
            if (p.allele_kind[a] == PH_KIND_NON_REF) continue;
            const uint8_t *s = p.allele_bases + p.allele_bases_off[a];
            if ((from_end ? s[p.allele_length[a] - at] : s[at]) != b) return false;
        }
        return true;
    };
    uint32_t size = min_len, s = 0, t = 0;
    while (size > 0 && same(true, t + 1)) ++t, --size;                 // alignment_utils.rs:608-614: bases[end - 1]
    while (size > 0 && same(false, s)) ++s, --size;                    // :616-622: bases[start]
    // :626-636 with max_shift == 0: start_shift is -s, so the loop runs while s > 0.  bases[start - 1] and bases[end - 1]; a range
    // keeps its length, and with s >= 1 its end - 1 is at least 0
    while (s > 0 && same(false, s - 1) && same(true, t + 1)) --s, ++t;
    const bool empty_allele = size == 0;                               // variant_context_utils.rs:993
    const bool restore_one_base_at_end = empty_allele && s == 0;       // :994; restore_one_base_at_start moves the start only,
    return restore_one_base_at_end ? t - 1 : t;                        // which trim_forward == false leaves where it is (:1011)
}

__global__ __launch_bounds__(PH_THREADS) void phase_trim_kernel(const PhaseParams p) {
    const uint32_t e = blockIdx.x * PH_THREADS + threadIdx.x;
    if (e >= p.n_events) return;
    const CallAlleles c = call_of(p, e);
    if (!c.C) {
        p.call_rev_trim[e] = 0;
        p.call_end[e] = -1;
        return;
    }
    // make_annotated_call trims only a call that lost alleles (haplotype_caller_genotyping_engine.rs:482-488)
    const uint32_t rev = (p.flags & PH_NO_TRIM) || c.C == c.A ? 0 : reverse_trim(p, c);
    p.call_rev_trim[e] = rev;
    p.call_end[e] = p.vc_start[e] + (int64_t)(p.allele_length[c.a0] - rev) - 1;   // :1063-1066 with the start where it was
}

// haplotype_caller_genotyping_engine.rs:394-405 as written: allele_mapper is keyed by the merged context's allele index and
// is asked for the POSITIONS 0..C_e of the call's list, so the haplotypes of the merged alleles 0..C_e are the called ones.
__global__ __launch_bounds__(PH_THREADS) void phase_called_kernel(const PhaseParams p) {
    const uint32_t t = blockIdx.x * PH_THREADS + threadIdx.x;
    const uint32_t e = t / 64u, lane = t % 64u;
    if (e >= p.n_events) return;
    const uint32_t C = p.call_allele_off[e + 1] - p.call_allele_off[e];
    if (!C) return;
    const uint32_t g = p.event_region[e], nh = p.region_hap_off[g + 1] - p.region_hap_off[g];
    const int32_t *map = p.event_hap_allele + p.event_map_off[e];
    for (uint32_t base = 0; base < nh; base += 64u) {
        const uint32_t h = base + lane;
        const int32_t a = h < nh ? map[h] : -1;
        const unsigned long long word = __ballot(a >= 0 && (uint32_t)a < C);
        if (lane == 0 && word) atomicOr(p.region_called + (size_t)g * PH_WORDS + base / 64u, word);
    }
}

__global__ __launch_bounds__(PH_THREADS) void phase_match_kernel(const PhaseParams p) {
    const uint32_t t = blockIdx.x * PH_THREADS + threadIdx.x;
    const uint32_t e = t / 64u, lane = t % 64u;
    if (e >= p.n_events) return;
    const CallAlleles c = call_of(p, e);
    const uint32_t g = p.event_region[e], h0 = p.region_hap_off[g], nh = p.region_hap_off[g + 1] - h0;
    // construct_haplotype_mapping (assembly_based_caller_utils.rs:1274-1310): exactly one site-specific alternate allele -- not
    // the reference, not '*', not <NON_REF> (:1343-1348) -- or the empty set
    uint32_t n_site = 0, alt = 0;
    for (uint32_t k = 1; k < c.C; ++k) {
        const uint32_t a = c.a0 + p.call_allele[c.c0 + k];
        if (p.allele_kind[a] == PH_KIND_PLAIN) {
            if (!n_site) alt = a;
            ++n_site;
        }
    }
    const bool mapped = c.C && n_site == 1;
    const uint8_t *alt_bases = mapped ? p.allele_bases + p.allele_bases_off[alt] : nullptr;
    const uint32_t alt_len = mapped ? p.allele_length[alt] - p.call_rev_trim[e] : 0;   // the trimmed allele: no base is copied
    const int64_t start = p.vc_start[e];
    uint32_t count = 0;
    for (uint32_t base = 0; base < nh; base += 64u) {
        const uint32_t h = base + lane;
        bool in = false;
        if (mapped && h < nh && ((p.region_called[(size_t)g * PH_WORDS + base / 64u] >> lane) & 1ull)) {
            // the haplotype's events ascend by start, one per start: the event at the call's start, if there is one
            uint32_t lo = p.hap_event_off[h0 + h], hi = p.hap_event_off[h0 + h + 1];
            const uint32_t end = hi;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (p.hap_event_start[mid] < start) lo = mid + 1;
                else hi = mid;
            }
            if (lo < end && p.hap_event_start[lo] == start) {
                const uint32_t b0 = p.hap_event_alt_off[lo], len = p.hap_event_alt_off[lo + 1] - b0;
                in = len == alt_len;
                for (uint32_t i = 0; in && i < len; ++i) in = p.hap_event_alt[b0 + i] == alt_bases[i];
            }
        }
        const unsigned long long word = __ballot(in);
        count += (uint32_t)__popcll(word);
        if (lane == 0) p.sets[(size_t)e * PH_WORDS + base / 64u] = word;
        if (p.hap_in_call && h < nh) p.hap_in_call[p.event_map_off[e] + h] = in ? 1 : 0;
    }
    if (lane == 0) p.phase_n_haps[e] = count;
}

__device__ inline unsigned long long wave_or(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d, 64);
    return v;
}

// construct_phase_set_mapping (assembly_based_caller_utils.rs:1109-1265), one wave per region.  i is serial.  Inside one i the
// reference's j loop depends on its own order in one place only: while i is unmapped, the FIRST related j decides -- mapped:
// the mapping is cleared and the function returns (:1180-1183, :1223-1226); unmapped: a new group with i (:1191-1194, :1228-1235).
// From then on i is mapped, and a related j either joins (unmapped, :1202-1207, :1237-1252) or is left alone (mapped).  Whether j
// is related to i is a function of S_i, S_j and total alone, and an iteration writes the entries of i and of its own j only.
// So the lanes take 64 j at a time, a ballot finds the first related one, and every related unmapped j joins at once.
// "Together" is (|Si| == |Sj| and Sj subset of Si) or |Sj| == total.  The reference's middle clause tests
// call_haplotypes_available_for_phasing, a set that is created empty and only ever retain()ed: it is false for every non-empty
// Sj, and it is left out here as it is without effect there.
__global__ __launch_bounds__(64) void phase_link_kernel(const PhaseParams p) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t e0 = p.region_event_off[g], ne = p.region_event_off[g + 1] - e0;
    const uint32_t nh = p.region_hap_off[g + 1] - p.region_hap_off[g], words = (nh + 63u) / 64u;
    uint32_t total = 0;                                                // :1114-1120: the union of the sets
    for (uint32_t w = 0; w < words; ++w) {
        unsigned long long acc = 0;
        for (uint32_t e = lane; e < ne; e += 64u) acc |= p.sets[(size_t)(e0 + e) * PH_WORDS + w];
        total += (uint32_t)__popcll(wave_or(acc));
    }
    for (uint32_t e = lane; e < ne; e += 64u) {
        p.phase_group[e0 + e] = -1;
        p.phase_gt[e0 + e] = 0;
    }
    __syncthreads();
    uint32_t counter = 0;                                              // unique_counter
    bool aborted = false;
    for (uint32_t i = 0; i + 1 < ne && !aborted; ++i) {
        const uint32_t ni = p.phase_n_haps[e0 + i];
        if (!ni) continue;                                             // :1134 (uniform: no barrier is skipped by part of the wave)
        unsigned long long si[PH_WORDS];
#pragma unroll
        for (uint32_t w = 0; w < PH_WORDS; ++w) si[w] = w < words ? p.sets[(size_t)(e0 + i) * PH_WORDS + w] : 0ull;
        int32_t i_group = p.phase_group[e0 + i];
        uint32_t i_gt = p.phase_gt[e0 + i];
        for (uint32_t base = i + 1; base < ne; base += 64u) {
            const uint32_t j = base + lane;
            const uint32_t nj = j < ne ? p.phase_n_haps[e0 + j] : 0;
            bool together = false, apart = false;
            if (nj) {                                                  // :1155
                uint32_t inter = 0;
#pragma unroll
                for (uint32_t w = 0; w < PH_WORDS; ++w)   // (a constant trip count keeps si in registers)
                    if (w < words) inter += (uint32_t)__popcll(si[w] & p.sets[(size_t)(e0 + j) * PH_WORDS + w]);
                together = (ni == nj && inter == nj) || nj == total;   // :1163-1173
                apart = !together && ni + nj == total && inter == 0;   // :1208-1217
            }
            const bool related = together || apart;
            const unsigned long long mask = __ballot(related);
            if (!mask) continue;
            if (i_group < 0) {
                const uint32_t first = base + (uint32_t)__ffsll((long long)mask) - 1u;
                if (p.phase_group[e0 + first] >= 0) {                  // another variant is in phase with the comp but not with the call
                    aborted = true;
                    break;
                }
                i_group = (int32_t)counter++;
                i_gt = 0;                                              // PHASE_01, also for a homozygous call (:1185-1190)
                if (lane == 0) {
                    p.phase_group[e0 + i] = i_group;
                    p.phase_gt[e0 + i] = 0;
                    p.group_leader[e0 + (uint32_t)i_group] = e0 + i;   // every later member has a larger index: i leads the group
                }
            }
            if (related && p.phase_group[e0 + j] < 0) {                // the first related j of a new group among them
                p.phase_group[e0 + j] = i_group;
                p.phase_gt[e0 + j] = (uint8_t)(together ? i_gt : 1u - i_gt);
            }
        }
        __syncthreads();                                               // the entries the lanes wrote are read by all as i goes on
    }
    if (aborted) {                                                     // phase_set_mapping.clear(): nothing in the region is phased
        __syncthreads();
        for (uint32_t e = lane; e < ne; e += 64u) {
            p.phase_group[e0 + e] = -1;
            p.phase_gt[e0 + e] = 0;
        }
    }
    if (lane == 0) {
        p.region_alt_haps[g] = total;
        p.region_phase_flags[g] = aborted ? PH_ABORTED : 0u;
    }
}

// construct_phase_groups and phase_vc (assembly_based_caller_utils.rs:1000-1083)
__global__ __launch_bounds__(PH_THREADS) void phase_apply_kernel(const PhaseParams p) {
    const uint64_t t = (uint64_t)blockIdx.x * PH_THREADS + threadIdx.x;
    const uint32_t per_event = p.gt ? max(p.n_samples, 1u) : 1u;
    const uint64_t e64 = t / per_event;
    if (e64 >= p.n_events) return;
    const uint32_t e = (uint32_t)e64, s = (uint32_t)(t % per_event);
    const CallAlleles c = call_of(p, e);
    const int32_t group = p.phase_group[e];
    if (s == 0) {
        const int32_t leader = group >= 0 ? (int32_t)p.group_leader[p.region_event_off[p.event_region[e]] + (uint32_t)group] : -1;
        p.phase_leader[e] = leader;
        p.phase_set[e] = leader >= 0 ? p.vc_start[leader] : -1;        // :1028: the start of the group's first call
    }
    if (!p.gt || s >= p.n_samples) return;
    const uint64_t at = (uint64_t)e * p.n_samples + s;
    const int32_t *gt = p.gt + at * p.ploidy;
    int32_t *out = p.gt_phased + at * p.ploidy;
    if (!c.C) {
        p.is_phased[at] = 0;
        for (uint32_t k = 0; k < p.ploidy; ++k) out[k] = -1;
        return;
    }
    bool reversed = false;
    if (group >= 0) {
        // determine_type (genotype_builder.rs:399-441): Het is no no-call allele and two different ones; a context's alleles
        // are distinct, so the indices decide
        bool no_call = false, multiple = false;
        for (uint32_t k = 0; k < p.ploidy; ++k) {
            no_call |= gt[k] < 0;
            multiple |= gt[k] != gt[0];
        }
        if (!no_call && multiple) {                                    // ploidy >= 2 here: the index below exists
            const int32_t al = gt[p.phase_gt[e] == 0 ? 1 : 0];        // alt_allele_index: 1 for 0|1, 0 for 1|0
            const bool site_specific = al != 0 && p.allele_kind[c.a0 + p.call_allele[c.c0 + (uint32_t)al]] == PH_KIND_PLAIN;
            reversed = !site_specific;                                 // :1064-1067
        }
    }
    p.is_phased[at] = group >= 0 ? 1 : 0;
    for (uint32_t k = 0; k < p.ploidy; ++k) out[k] = gt[reversed ? p.ploidy - 1u - k : k];
}

}  // namespace

hipError_t launch_phase(const PhaseParams &p, hipStream_t stream) {
    if (!p.n_regions) return hipSuccess;
    const auto blocks = [](uint64_t threads) { return dim3((uint32_t)((threads + PH_THREADS - 1) / PH_THREADS)); };
    if (p.n_events) {
        hipError_t e = hipMemsetAsync(p.region_called, 0, sizeof(unsigned long long) * PH_WORDS * (size_t)p.n_regions, stream);
        if (e != hipSuccess) return e;
        phase_trim_kernel<<<blocks(p.n_events), PH_THREADS, 0, stream>>>(p);
        phase_called_kernel<<<blocks((uint64_t)p.n_events * 64u), PH_THREADS, 0, stream>>>(p);
        phase_match_kernel<<<blocks((uint64_t)p.n_events * 64u), PH_THREADS, 0, stream>>>(p);
    }
    phase_link_kernel<<<dim3(p.n_regions), 64, 0, stream>>>(p);
    if (p.n_events) phase_apply_kernel<<<blocks((uint64_t)p.n_events * (p.gt ? (p.n_samples ? p.n_samples : 1u) : 1u)), PH_THREADS, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace phmm
