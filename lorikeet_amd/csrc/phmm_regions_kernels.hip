// Assembly regions for gfx950 (phmm_assembly_regions, include/phmm.h): ActivityProfile::pop_ready_assembly_regions
// (src/activity_profile/activity_profile.rs:371-668) over many band-passed state lists, and the reads a fetch of each region's
// padded span returns (src/assembly/assembly_region_iterator.rs:54-159 without BAM I/O and read_is_filtered).  Integers, f32
// compares and ballots; the only arithmetic in floating point is one division per region and one per read.
//
//   regions_class_kernel    a lane per state: three bit planes packed by ballot into 64-bit words per profile -- prob > threshold,
//                           the local-minimum test p[i] <= p[i+1] && p[i] < p[i-1] for 1 <= i < len - 1, prob > 0.05
//   regions_cut_kernel      one wave per profile, the only serial part: per region the boundary is the first differing bit over at
//                           most ceil(max_region_size / 64) + 1 words, 64 words a pass; the cut site a wave reduction keyed
//                           (value, then higher index) over the candidates of the minimum plane.  Writes a region's first state,
//                           its states and flags into the profile's slab, the count and the status
//   regions_scan_kernel     one workgroup: profile_region_off
//   regions_span_kernel     one wave per region: spans, padding, the density as a popcount over the third plane
//   regions_read_kernel     one wave per read: the reference length of its CIGAR, the sum of its qualities
//   regions_pmax_kernel     one wave per (window, sample) group: the running maximum of the reads' ends, a wave scan with a carry
//   regions_count_kernel    one wave per (region, sample): two binary searches bound the candidates, ballots count the overlaps
//   regions_offsets_kernel  one workgroup: region_read_off, the sum in 64 bits
//   regions_finish_kernel   a lane per region: its reads over all samples, the flags
//   regions_members_kernel  one wave per (region, sample): the overlapping reads in input order, ballot-compacted
// No atomics; every element has one writer.
#include "phmm_regions_internal.hpp"

#include <cfloat>

namespace phmm {

namespace {

__device__ __forceinline__ uint32_t popc64(uint64_t v) { return (uint32_t)__popcll((unsigned long long)v); }
__device__ __forceinline__ uint64_t bits_below(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }  // bits [0, n)

// the largest k with off[k] <= i, off [n + 1] ascending from 0 (empty entries repeat a value: the last of them is taken)
__device__ __forceinline__ uint32_t owner_of(const uint32_t *off, uint32_t n, uint32_t i) {
    uint32_t lo = 0, hi = n;  // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int m = 32; m; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, unsigned d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int m = 32; m; m >>= 1) v += shfl_xor64(v, m);
    return v;
}

// ---- the planes ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(REG_CLASS_THREADS) void regions_class_kernel(RegionsParams p) {
    const uint32_t lane = threadIdx.x & 63u, word = blockIdx.x * (REG_CLASS_THREADS / 64) + (threadIdx.x >> 6);
    if (word >= p.n_words) return;  // (whole waves leave)
    const uint32_t k = owner_of(p.word_off, p.n_profiles, word);
    const uint32_t n = p.len[k], i = (word - p.word_off[k]) * 64 + lane;
    const float *q = p.prob + p.first[k];
    bool active = false, minimum = false, dense = false;
    if (i < n) {
        const float v = q[i];
        active = v > p.threshold;  // is_active_prob() > active_prob_threshold (:465, :631); a NaN is inactive
        dense = v > REG_DENSITY_TOLERANCE;
        // is_minimum (:660-668) where it does not depend on the drain point: never the last state of the list
        if (i >= 1 && i + 1 < n) minimum = v <= q[i + 1] && v < q[i - 1];
    }
    const uint64_t a = __ballot(active), m = __ballot(minimum), d = __ballot(dense);
    if (lane == 0) {
        p.plane_active[word] = a;
        p.plane_min[word] = m;
        p.plane_dense[word] = d;
    }
}

// ---- pop_ready_assembly_regions (:371-412), one wave per profile --------------------------------------------------------------
__global__ __launch_bounds__(64) void regions_cut_kernel(RegionsParams p) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    const uint32_t n = p.len[k], slab = p.state_off[k];
    const uint64_t *act = p.plane_active + p.word_off[k], *mins = p.plane_min + p.word_off[k];
    const float *q = p.prob + p.first[k];
    const uint64_t start0 = p.start[k], stop = p.stop[k], contig = p.contig[k];
    uint32_t cur = 0, count = 0;
    uint64_t prev_start = 0;
    int32_t status = 0;
    while (cur < n) {  // (an empty list: pop_next_ready_assembly_region returns None, :436)
        const uint32_t rem = n - cur;
        // :384-392; the list is not empty here, so region_stop_loc is still the last ADDED state
        const bool force = count && prev_start != stop + 1;
        if (!force && (uint64_t)rem < (uint64_t)p.max_size + p.max_prop) break;  // :552-558
        const bool is_active = (act[cur >> 6] >> (cur & 63u)) & 1u;              // :465
        // find_first_activity_boundary (:621-640): the first state in [0, min(rem, max)) that differs
        const uint32_t limit = rem < p.max_size ? rem : p.max_size;
        const uint32_t w0 = cur >> 6, w1 = (cur + limit - 1) >> 6;               // limit >= 1
        uint32_t e = limit;
        for (uint32_t base = w0; base <= w1; base += 64) {
            const uint32_t w = base + lane;
            uint64_t x = 0;
            if (w <= w1) {
                x = act[w] ^ (is_active ? ~0ull : 0ull);
                if (w == w0) x &= ~bits_below(cur & 63u);
                if (w == w1) x &= bits_below(((cur + limit - 1) & 63u) + 1);
            }
            const uint64_t hit = __ballot(x != 0);
            if (hit) {
                const uint32_t src = (uint32_t)__builtin_ctzll(hit);
                e = (base + src) * 64 + (uint32_t)__builtin_ctzll(shfl64(x, (int)src)) - cur;
                break;
            }
        }
        if (is_active && e == p.max_size) {  // find_best_cut_site (:582-605)
            if (e < p.min_size) {            // the assertion :583-586
                status = REG_STATUS_MIN_REGION_SIZE;
                break;
            }
            // i from e - 1 down to min_size with `cur < min_p && is_minimum(i)`, min_p from f32::MAX: the smallest value wins,
            // the highest index among equals; a NaN, +inf and f32::MAX never do
            float best = FLT_MAX;
            uint32_t best_i = 0;
            bool have = false;
            for (uint32_t i = p.min_size + lane; i < e; i += 64) {
                const uint32_t s = cur + i;  // index in the whole list; i >= 1, so s - 1 is still in the remaining list
                const bool is_min = i >= 1 && s != n - 1 && ((mins[s >> 6] >> (s & 63u)) & 1u);
                const float v = q[s];
                if (is_min && v < FLT_MAX && (!have || v <= best)) {  // (i ascends inside a lane: an equal later one wins)
                    best = v;
                    best_i = i;
                    have = true;
                }
            }
            for (int m = 32; m; m >>= 1) {
                const float ob = __shfl_xor(best, m, 64);
                const uint32_t oi = (uint32_t)__shfl_xor((int)best_i, m, 64);
                const bool oh = __shfl_xor((int)have, m, 64) != 0;
                if (oh && (!have || ob < best || (ob == best && oi > best_i))) {
                    best = ob;
                    best_i = oi;
                    have = true;
                }
            }
            if (have) e = best_i + 1;  // else min_i stays e - 1
        }
        if (e == 0) break;  // checked_sub (:568)
        const uint64_t start = start0 + cur;
        if (start > contig - 1) {  // SimpleInterval::size underflows (:508)
            status = REG_STATUS_START_PAST_CONTIG;
            break;
        }
        if (lane == 0) {
            p.slab_first[slab + count] = cur;
            p.slab_len[slab + count] = e;
            p.slab_flags[slab + count] = (is_active ? REG_ACTIVE : 0u) | (force ? REG_FORCED : 0u);
        }
        ++count;
        prev_start = start;
        cur += e;
    }
    if (lane == 0) {
        p.profile_count[k] = count;
        p.profile_status[k] = status;
    }
}

// an exclusive scan of v [n] into off [n + 1] by one workgroup; returns the total (64 bits: a sum may pass 2^32)
__device__ uint64_t regions_block_scan(const uint32_t *v, uint32_t *off, uint32_t n, uint64_t *sums) {
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + REG_SCAN_THREADS - 1) / REG_SCAN_THREADS;  // a run of `per` entries a thread
    const uint32_t b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    uint64_t mine = 0;
    for (uint32_t i = b; i < e; ++i) mine += v[i];
    sums[t] = mine;
    __syncthreads();
    if (t == 0) {
        uint64_t run = 0;
        for (uint32_t i = 0; i < REG_SCAN_THREADS; ++i) {
            const uint64_t s = sums[i];
            sums[i] = run;
            run += s;
        }
        sums[REG_SCAN_THREADS] = run;
    }
    __syncthreads();
    uint64_t run = sums[t];
    for (uint32_t i = b; i < e; ++i) {
        off[i] = (uint32_t)run;
        run += v[i];
    }
    const uint64_t total = sums[REG_SCAN_THREADS];
    if (t == 0) off[n] = (uint32_t)total;
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(REG_SCAN_THREADS) void regions_scan_kernel(RegionsParams p) {
    __shared__ uint64_t sums[REG_SCAN_THREADS + 1];
    regions_block_scan(p.profile_count, p.profile_region_off, p.n_profiles, sums);
}

// ---- AssemblyRegion::new (:495-519, assembly_region.rs:73-98, :169-189), one wave per region ------------------------------------
__global__ __launch_bounds__(64) void regions_span_kernel(RegionsParams p) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint32_t k = owner_of(p.profile_region_off, p.n_profiles, r);
    const uint32_t j = p.state_off[k] + (r - p.profile_region_off[k]);
    const uint32_t first = p.slab_first[j], n = p.slab_len[j];
    const uint64_t contig = p.contig[k];
    const uint64_t start = p.start[k] + first;
    const uint64_t last = start + (n - 1), end = last < contig - 1 ? last : contig - 1;  // min(start + offset, contig_len - 1)
    // the drained states with prob > 0.05: all n of them, also where the span was clipped
    const uint64_t *dense = p.plane_dense + p.word_off[k];
    const uint32_t w0 = first >> 6, w1 = (first + n - 1) >> 6;
    uint32_t c = 0;
    for (uint32_t w = w0 + lane; w <= w1; w += 64) {
        uint64_t x = dense[w];
        if (w == w0) x &= ~bits_below(first & 63u);
        if (w == w1) x &= bits_below(((first + n - 1) & 63u) + 1);
        c += popc64(x);
    }
    c = wave_sum(c);
    if (lane) return;
    const uint64_t size = end - start + 1;  // start <= contig - 1 (regions_cut_kernel)
    p.region_density[r] = (float)(uint64_t)c / (float)size;  // count as f32 / size as f32
    // make_padded_span: saturating start; trim_interval_to_contig: min(contig_length, stop), None when the start is past the contig
    const uint64_t ps = p.extension > start ? 0 : start - p.extension, pe = end + p.extension < contig ? end + p.extension : contig;
    const bool none = ps > contig;
    p.region_start[r] = start;
    p.region_end[r] = end;
    p.region_padded_start[r] = none ? start : ps;
    p.region_padded_end[r] = none ? end : pe;
    p.region_states[r] = n;
    p.region_flags0[r] = p.slab_flags[j];
    p.region_profile[r] = k;
}

// ---- per read: bam_cigar2rlen over M, D, N, = and X; the depth cap's key (assembly_region_iterator.rs:143-147) -----------------
__global__ __launch_bounds__(REG_CLASS_THREADS) void regions_read_kernel(RegionsParams p) {
    const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * (REG_CLASS_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= p.n_reads) return;
    uint64_t reflen = 0, qsum = 0;
    for (uint32_t c = p.cigar_off[r] + lane; c < p.cigar_off[r + 1]; c += 64) {
        const uint32_t op = p.cigar[c] & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += p.cigar[c] >> 4;
    }
    const uint32_t b0 = p.read_off[r], b1 = p.read_off[r + 1];
    for (uint32_t b = b0 + lane; b < b1; b += 64) qsum += p.quals[b];
    reflen = wave_sum64(reflen);
    qsum = wave_sum64(qsum);
    if (lane) return;
    p.read_end[r] = p.read_pos[r] + (int64_t)(reflen ? reflen : 1);  // exclusive; htslib gives a read without reference bases one
    // the sum of u8 as f64 is exact in any order below 2^53; a read without qualities gives 0 / 0 = NaN
    p.read_mean_qual[r] = (double)qsum / (double)(uint64_t)(b1 - b0);
}

// ---- per group: read_pmax[r] = the largest end among the group's reads up to r ---------------------------------------------------
__global__ __launch_bounds__(64) void regions_pmax_kernel(RegionsParams p) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t r0 = p.group_read_off[g], r1 = p.group_read_off[g + 1];
    int64_t carry = INT64_MIN;
    for (uint32_t base = r0; base < r1; base += 64) {
        const uint32_t r = base + lane;
        int64_t v = r < r1 ? p.read_end[r] : INT64_MIN;
        for (unsigned d = 1; d < 64; d <<= 1) {
            const int64_t o = (int64_t)shfl_up64((uint64_t)v, d);
            if (lane >= d && o > v) v = o;
        }
        if (carry > v) v = carry;
        if (r < r1) p.read_pmax[r] = v;
        carry = (int64_t)shfl64((uint64_t)v, 63);
    }
}

// the candidates of (region, sample): reads [lo, hi) of the group -- hi the first with pos > padded end (read_pos ascends), lo
// the first whose running maximum passes the padded start (no read before it reaches the span)
__device__ __forceinline__ void candidates(const RegionsParams &p, uint32_t r, uint32_t s, uint32_t *lo_out, uint32_t *hi_out) {
    const uint32_t g = p.window[p.region_profile[r]] * p.n_samples + s;
    const uint32_t r0 = p.group_read_off[g], r1 = p.group_read_off[g + 1];
    const int64_t ps = (int64_t)p.region_padded_start[r], pe = (int64_t)p.region_padded_end[r];
    uint32_t lo = r0, hi = r1;
    while (lo < hi) {  // the first read with pos > pe
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p.read_pos[mid] > pe) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t upper = lo;
    lo = r0, hi = upper;
    while (lo < hi) {  // the first read with pmax > ps
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p.read_pmax[mid] > ps) hi = mid;
        else lo = mid + 1;
    }
    *lo_out = lo;
    *hi_out = upper;
}

__global__ __launch_bounds__(64) void regions_count_kernel(RegionsParams p) {
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    const uint32_t r = pair / p.n_samples, s = pair % p.n_samples;
    uint32_t lo, hi;
    candidates(p, r, s, &lo, &hi);
    const int64_t ps = (int64_t)p.region_padded_start[r];
    uint32_t c = 0;
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        c += popc64(__ballot(i < hi && p.read_end[i] > ps));  // pos <= padded.end holds for every candidate
    }
    if (lane == 0) {
        p.pair_lo[pair] = lo;
        p.pair_hi[pair] = hi;
        p.pair_count[pair] = c;
    }
}

__global__ __launch_bounds__(REG_SCAN_THREADS) void regions_offsets_kernel(RegionsParams p) {
    __shared__ uint64_t sums[REG_SCAN_THREADS + 1];
    const uint64_t total = regions_block_scan(p.pair_count, p.region_read_off, p.n_regions * p.n_samples, sums);
    if (threadIdx.x == 0) *p.n_memberships = total;
}

__global__ __launch_bounds__(64) void regions_finish_kernel(RegionsParams p) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r >= p.n_regions) return;
    uint32_t n = 0;
    if (p.group_read_off) n = p.region_read_off[(r + 1) * p.n_samples] - p.region_read_off[r * p.n_samples];
    p.region_n_reads[r] = n;
    p.region_flags[r] = p.region_flags0[r] | (n > p.max_depth ? REG_OVER_DEPTH : 0u);  // records.len() > max_input_depth (:141)
}

__global__ __launch_bounds__(64) void regions_members_kernel(RegionsParams p) {
    const uint32_t pair = blockIdx.x, lane = threadIdx.x;
    const uint32_t r = pair / p.n_samples;
    const uint32_t lo = p.pair_lo[pair], hi = p.pair_hi[pair];
    const int64_t ps = (int64_t)p.region_padded_start[r];
    uint32_t at = p.region_read_off[pair];
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        const bool in = i < hi && p.read_end[i] > ps;
        const uint64_t hits = __ballot(in);
        if (in) p.region_reads[at + popc64(hits & bits_below(lane))] = i;
        at += popc64(hits);
    }
}

}  // namespace

hipError_t launch_regions_cut(const RegionsParams &p, hipStream_t stream) {
    if (!p.n_profiles) return hipSuccess;
    const uint32_t words = p.n_words;
    if (words) regions_class_kernel<<<(words + REG_CLASS_THREADS / 64 - 1) / (REG_CLASS_THREADS / 64), REG_CLASS_THREADS, 0, stream>>>(p);
    regions_cut_kernel<<<p.n_profiles, 64, 0, stream>>>(p);
    regions_scan_kernel<<<1, REG_SCAN_THREADS, 0, stream>>>(p);
    return hipGetLastError();
}

hipError_t launch_regions_spans(const RegionsParams &p, hipStream_t stream) {
    const bool reads = p.group_read_off != nullptr;
    if (p.n_regions) regions_span_kernel<<<p.n_regions, 64, 0, stream>>>(p);
    if (reads && p.n_reads) regions_read_kernel<<<(p.n_reads + REG_CLASS_THREADS / 64 - 1) / (REG_CLASS_THREADS / 64), REG_CLASS_THREADS, 0, stream>>>(p);
    if (reads && p.n_reads && p.n_groups) regions_pmax_kernel<<<p.n_groups, 64, 0, stream>>>(p);
    if (reads && p.n_regions) {
        regions_count_kernel<<<p.n_regions * p.n_samples, 64, 0, stream>>>(p);
        regions_offsets_kernel<<<1, REG_SCAN_THREADS, 0, stream>>>(p);
    }
    if (p.n_regions) regions_finish_kernel<<<(p.n_regions + 63) / 64, 64, 0, stream>>>(p);
    return hipGetLastError();
}

hipError_t launch_regions_members(const RegionsParams &p, hipStream_t stream) {
    if (p.group_read_off && p.n_regions) regions_members_kernel<<<p.n_regions * p.n_samples, 64, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace phmm
