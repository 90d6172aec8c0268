// Region trimming for gfx950 (phmm_trim_regions, include/phmm.h): what the reference's call_region does with the assembler's
// haplotypes before a likelihood is computed -- get_variation_events, AssemblyRegionTrimmer::trim, AssemblyResultSet::trim_to.
// Integer and byte work only; no floating point in this file (-ffp-contract=off comes with phmm_cigar_device.hpp).
//
//   events_hap_kernel    (phmm_events_kernels.hip, launch_event_maps) the event map of every haplotype, into the workspace
//   trim_span_kernel     one wave per region: the region's status is that of its first haplotype whose map failed; the lanes
//                        run over each haplotype's events 64 a pass (as events_region_kernel reads the workspace), four running
//                        extremes a lane, one wave reduction, the intersections
//   trim_hap_kernel      one lane per haplotype (as finalize_clip_kernel is a lane per read): Haplotype::trim.  The CIGAR walk
//                        of get_bases_covering_ref_interval is per element in closed form; the window of bases, the new CIGAR
//                        through the device Builder, the fate or the panic
//   trim_rank_kernel     one wave per haplotype i: against every surviving j of its region it compares the length, then the
//                        upper-cased bytes, 256 a pass (four loads a lane in flight) with ballots for the first differing
//                        lane.  It counts the smaller j and finds the class's representative.  Every pair needs its ORDER,
//                        which no fingerprint gives, so none is computed
//   trim_order_kernel    one workgroup per region: the first panic in input order; else the dense rank among representatives
//                        from those counts (integers in LDS), the fates, the set's variation and reference haplotype
//   trim_scan_kernel     one workgroup: the dense offsets (regions, then bases and CIGAR elements by output index)
//   trim_gather_kernel   one wave per output haplotype: the bases upper-cased (Haplotype::new), the CIGAR, the scalars
// No atomics; every element has one writer; every position comes from a prefix sum.
#include "phmm_trim_internal.hpp"

#include "phmm_cigar_device.hpp"

namespace phmm {

namespace {

using namespace cigdev;

__device__ __forceinline__ uint8_t upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
    for (int m = 32; m; m >>= 1) {
        const uint64_t o = shfl_xor64(v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
    for (int m = 32; m; m >>= 1) {
        const uint64_t o = shfl_xor64(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// ---- per region: AssemblyRegionTrimmer::trim (assembly_region_trimmer.rs:61-131), trim_with_padded_span ---------------------
__global__ __launch_bounds__(64) void trim_span_kernel(TrimParams p) {
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t h0 = p.region_hap_off[g], h1 = p.region_hap_off[g + 1];
    int32_t status = 0;  // build_event_maps_for_haplotypes stops at its first failing haplotype (call_region :1197-1204)
    for (uint32_t base = h0; base < h1 && !status; base += 64) {
        const uint32_t h = base + lane;
        const unsigned long long bad = __ballot(h < h1 && p.hap_status[h] < 0);
        if (bad) status = p.hap_status[base + (uint32_t)__builtin_ctzll(bad)];
    }
    const uint64_t rs = p.ref_start[g], as = p.active_start[g], ae = p.active_end[g], ps = p.padded_start[g], pe = p.padded_end[g];
    uint64_t mn = ~0ull, mx = 0, pmn = ~0ull, pmx = 0;
    bool any = false, bad_slice = false;
    const uint64_t ref_len = p.ref_off[g + 1] - p.ref_off[g];
    if (!status)
        for (uint32_t h = h0; h < h1; ++h) {
            const HapEvent *evs = p.ws_ev + p.ws_ev_off[h];
            const uint32_t n = p.hap_n_ev[h];
            for (uint32_t k = lane; k < n; k += 64) {
                const uint64_t vs = rs + evs[k].start, ve = rs + evs[k].end;
                if (!(as <= ve && vs <= ae)) continue;  // SimpleInterval::overlaps (simple_interval.rs:201-205, :341-343)
                any = true;
                const uint64_t pad = evs[k].type == EV_TYPE_INDEL ? p.pad_indel : p.pad_snp;  // vc.is_indel(): the cached type
                mn = vs < mn ? vs : mn;
                mx = ve > mx ? ve : mx;
                const uint64_t lo = vs > pad ? vs - pad : 0, hi = ve + pad;  // saturating_sub (:115)
                pmn = lo < pmn ? lo : pmn;
                pmx = hi > pmx ? hi : pmx;
                // TandemRepeat::get_num_tandem_repeat_units (src/annotator/tandem_repeat.rs:21-25) slices the reference bases from
                // start + 1 - padded span start for every indel before it returns None: a start in front of the padded span
                // underflows, an index behind the bases panics
                if (evs[k].type == EV_TYPE_INDEL && (vs + 1 < ps || vs + 1 - ps > ref_len)) bad_slice = true;
            }
        }
    any = __any(any);
    if (__any(bad_slice)) status = TRIM_REPEAT_SLICE, any = false;
    mn = wave_min(mn), pmn = wave_min(pmn), mx = wave_max(mx), pmx = wave_max(pmx);
    if (lane) return;
    uint64_t v0 = 0, v1 = 0, s0 = 0, s1 = 0, a0 = 0, a1 = 0, q0 = 0, q1 = 0;
    if (any) {
        v0 = mn > as ? mn : as, v1 = mx < ae ? mx : ae;      // variant_span = [min start, max end] & active span (:93-94)
        s0 = pmn > ps ? pmn : ps, s1 = pmx < pe ? pmx : pe;  // padded_variant_span (:119-120)
        a0 = as > v0 ? as : v0, a1 = ae < v1 ? ae : v1;      // trim_with_padded_span (assembly_region.rs:328-329)
        q0 = ps > s0 ? ps : s0, q1 = pe < s1 ? pe : s1;
    }
    p.region_status[g] = status;
    p.variation[g] = any ? TRIM_VARIATION_SPAN : 0;
    p.variant_start[g] = v0, p.variant_end[g] = v1, p.span_start[g] = s0, p.span_end[g] = s1;
    p.new_active_start[g] = a0, p.new_active_end[g] = a1, p.new_padded_start[g] = q0, p.new_padded_end[g] = q1;
}

// ---- per haplotype: Haplotype::trim (haplotype.rs:149-236) ------------------------------------------------------------------
__global__ __launch_bounds__(64) void trim_hap_kernel(TrimParams p) {
    const uint32_t h = blockIdx.x * 64 + threadIdx.x;
    if (h >= p.n_haps) return;
    const uint32_t g = p.hap_region[h];
    uint32_t first = 0, wlen = 0, n_new = 0, start_out = 0;
    int32_t panic = 0, fate = TRIM_FATE_NOT_TRIMMED;
    if (p.region_status[g] == 0 && (p.variation[g] & TRIM_VARIATION_SPAN)) {
        const uint64_t ps = p.new_padded_start[g], pe = p.new_padded_end[g], ls = p.loc_start[h], le = p.loc_end[h];
        const uint32_t *cig = p.cigar + p.cigar_off[h], n = p.cigar_off[h + 1] - p.cigar_off[h];
        const uint64_t L = p.hap_off[h + 1] - p.hap_off[h];
        [&] {
            if (!(ls <= ps && le >= pe)) return (void)(panic = TRIM_LOCATION);  // "Can only trim a Haplotype to a containing span."
            const uint64_t new_start = ps - ls, new_stop = new_start + pe - ps;
            // get_bases_covering_ref_interval (alignment_utils.rs:759-843)
            uint64_t read_len = 0;
            for (uint32_t i = 0; i < n; ++i) read_len += read_len_of(cig[i]);
            if (read_len != L) return (void)(panic = TRIM_LENGTH);  // "Mismatch between length in reference bases and cigar length"
            uint64_t ref_pos = 0, bases_pos = 0, b_start = 0, b_stop = 0;
            bool have_start = false, have_stop = false, done = false;
            for (uint32_t i = 0; i < n && !done; ++i) {
                const int op = op_of(cig[i]);
                const uint64_t len = len_of(cig[i]);
                const bool start_in = new_start >= ref_pos && new_start < ref_pos + len, stop_in = new_stop >= ref_pos && new_stop < ref_pos + len;
                if (op == OP_I) {
                    bases_pos += len;
                } else if (op == OP_M || op == OP_EQ || op == OP_X) {
                    if (start_in) b_start = bases_pos + (new_start - ref_pos), have_start = true;  // the start test first (:796-798)
                    if (stop_in) {
                        b_stop = bases_pos + (new_stop - ref_pos), have_stop = done = true;
                        bases_pos = b_stop, ref_pos = new_stop;
                    } else {
                        ref_pos += len, bases_pos += len;
                    }
                } else if (op == OP_D) {
                    if (start_in || stop_in) return (void)(fate = TRIM_FATE_CUT_IN_DELETION);  // either bound (:811-814)
                    ref_pos += len;
                } else {
                    return (void)(panic = TRIM_OPERATOR);  // "Unsupported operator"
                }
            }
            if (ref_pos == new_start) b_start = bases_pos, have_start = true;  // the two tests behind the loop (:824-831)
            if (ref_pos == new_stop) b_stop = bases_pos, have_stop = true;
            if (!have_start || !have_stop) return (void)(panic = TRIM_NOT_FOUND);  // "Never found start or stop"
            const uint64_t hi = b_stop + 1 < L ? b_stop + 1 : L;  // min(stop + 1, len) (:841)
            if (hi <= b_start) return (void)(fate = TRIM_FATE_EMPTY);  // new_bases.len() == 0 (haplotype.rs:180-182)
            // trim_cigar_by_reference(cigar, new_start, new_stop) (:187-192)
            Builder T;
            T.init(p.ws_cigar_a + p.cigar_off[h], n, true);
            const int st = trim_by_reference(T, cig, n, new_start, new_stop, nullptr, nullptr);
            // (CIGAR_ERR_PANIC, the CIGAR ending in front of `end`, cannot come once the walk above has found the stop; a builder Err
            // can: an insertion behind a right soft clip that sits at end + 1)
            if (st != CIGAR_OK) return (void)(panic = st == CIGAR_ERR_PANIC ? TRIM_NOT_FOUND : TRIM_BUILDER);
            // T.n >= 1 here: Builder::make returns CIGAR_ERR_NONE / CIGAR_ERR_EMPTY for a builder without elements
            const bool leading = !on_ref(op_of(T.el[0])), trailing = !on_ref(op_of(T.el[T.n - 1]));
            const uint32_t keep0 = leading ? 1 : 0, keep1 = T.n - (trailing ? 1 : 0);
            if (keep1 <= keep0) return (void)(fate = TRIM_FATE_ALL_INSERTION);  // "edge case of entire cigar is insertion" (:202-205)
            uint32_t *out = p.ws_cigar_b + p.cigar_off[h];
            if (!(leading || trailing)) {
                for (uint32_t i = 0; i < T.n; ++i) out[i] = T.el[i];
                n_new = T.n;
            } else {  // CigarBuilder::new(false) over the kept elements (:211-223)
                Builder U;
                U.init(out, n, false);
                for (uint32_t i = keep0; i < keep1; ++i)
                    if (U.add(T.el[i]) != CIGAR_OK) return (void)(panic = TRIM_BUILDER);
                if (U.make() != CIGAR_OK) return (void)(panic = TRIM_BUILDER);
                n_new = U.n;
            }
            first = (uint32_t)b_start, wlen = (uint32_t)(hi - b_start);
            start_out = (uint32_t)(new_start + p.hap_start[h]);  // alignment_start_hap_wrt_ref (:231)
            fate = 0;
        }();
        // trim_down_haplotypes (assembly_result_set.rs:487-490): None for the reference haplotype panics
        if (!panic && fate < 0 && p.is_ref[h]) panic = TRIM_REF_ELIMINATED;
    }
    p.win_first[h] = first;
    p.win_len[h] = fate == 0 ? wlen : 0;
    p.new_n_cigar[h] = fate == 0 ? n_new : 0;
    p.new_start[h] = start_out;
    p.hap_panic[h] = panic;
    p.hap_fate[h] = fate;
    p.hap_dup_of[h] = TRIM_NONE;
}

// ---- trim_down_haplotypes' BTreeMap (assembly_result_set.rs:465-499), Haplotype's Ord (haplotype.rs:269-284) -----------------
// (length, upper-cased bytes) of a against b: -1, 0, 1; the same in every lane.  256 bytes a pass: four loads a lane in flight,
// the ballots looked at in byte order.
__device__ __forceinline__ int compare(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, uint32_t lane) {
    if (la != lb) return la < lb ? -1 : 1;
    for (uint32_t c = 0; c < la; c += 256) {
        bool d[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t o = c + q * 64 + lane;
            d[q] = o < la && upper(a[o]) != upper(b[o]);
        }
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const unsigned long long diff = __ballot(d[q]);
            if (diff) {
                const uint32_t k = c + q * 64 + (uint32_t)__builtin_ctzll(diff);
                return upper(a[k]) < upper(b[k]) ? -1 : 1;
            }
        }
    }
    return 0;
}

// a wave per haplotype i: the surviving haplotypes of its region below it, and its class's representative
__global__ __launch_bounds__(64) void trim_rank_kernel(TrimParams p) {
    const uint32_t h = blockIdx.x, lane = threadIdx.x, g = p.hap_region[h];
    const uint32_t h0 = p.region_hap_off[g], nh = p.region_hap_off[g + 1] - h0, i = h - h0;
    uint32_t below = TRIM_NONE, first_eq = TRIM_NONE, last_ref_eq = TRIM_NONE;
    if (p.region_status[g] == 0 && (p.variation[g] & TRIM_VARIATION_SPAN) && p.hap_fate[h] == 0) {
        const uint8_t *a = p.hap_bases + p.hap_off[h] + p.win_first[h];
        const uint32_t la = p.win_len[h];
        below = 0;
        for (uint32_t j = 0; j < nh; ++j) {
            if (p.hap_fate[h0 + j] != 0) continue;
            const int c = j == i ? 0 : compare(p.hap_bases + p.hap_off[h0 + j] + p.win_first[h0 + j], p.win_len[h0 + j], a, la, lane);
            below += c < 0;
            if (c == 0) {
                if (first_eq == TRIM_NONE) first_eq = j;
                if (p.is_ref[h0 + j]) last_ref_eq = j;  // an equal reference haplotype replaces key and value (:478-482)
            }
        }
    }
    if (lane == 0) {
        p.hap_below[h] = below;
        p.hap_rep[h] = last_ref_eq != TRIM_NONE ? last_ref_eq : first_eq;
    }
}

// a workgroup per region: the first panic in input order, else the dense ranks, the fates, what trim_to leaves of the set
__global__ __launch_bounds__(TRIM_RANK_THREADS) void trim_order_kernel(TrimParams p) {
    __shared__ uint32_t smaller[EV_MAX_HAPS], rep[EV_MAX_HAPS];  // per haplotype: surviving haplotypes below it; its class's representative
    __shared__ uint32_t first_panic;
    const uint32_t g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t h0 = p.region_hap_off[g], nh = p.region_hap_off[g + 1] - h0;
    if (p.region_status[g] < 0 || !(p.variation[g] & TRIM_VARIATION_SPAN)) {
        if (t == 0) p.region_n_out[g] = 0, p.out_region_ref_hap[g] = -1;
        return;
    }
    if (wave == 0) {  // the first haplotype in input order whose trim panics
        uint32_t at = TRIM_NONE;
        for (uint32_t base = 0; base < nh && at == TRIM_NONE; base += 64) {
            const uint32_t i = base + lane;
            const unsigned long long bad = __ballot(i < nh && p.hap_panic[h0 + i] < 0);
            if (bad) at = base + (uint32_t)__builtin_ctzll(bad);
        }
        if (lane == 0) first_panic = at;
    }
    for (uint32_t i = t; i < nh; i += TRIM_RANK_THREADS) smaller[i] = p.hap_below[h0 + i], rep[i] = p.hap_rep[h0 + i];
    __syncthreads();
    if (first_panic != TRIM_NONE) {
        for (uint32_t i = t; i < nh; i += TRIM_RANK_THREADS) p.hap_fate[h0 + i] = TRIM_FATE_NOT_TRIMMED;
        if (t == 0) {
            p.region_status[g] = p.hap_panic[h0 + first_panic];
            p.region_n_out[g] = 0;
            p.out_region_ref_hap[g] = -1;
        }
        return;
    }
    for (uint32_t i = t; i < nh; i += TRIM_RANK_THREADS) {
        if (smaller[i] == TRIM_NONE) continue;
        if (rep[i] != i) {
            p.hap_fate[h0 + i] = TRIM_FATE_DUPLICATE;
            p.hap_dup_of[h0 + i] = rep[i];
            continue;
        }
        uint32_t rank = 0;  // the classes below this one: their representatives are as many
        for (uint32_t j = 0; j < nh; ++j) rank += smaller[j] != TRIM_NONE && rep[j] == j && smaller[j] < smaller[i];
        p.hap_fate[h0 + i] = (int32_t)rank;
    }
    if (t == 0) {
        uint32_t n_out = 0, top = 0;
        int32_t ref_at = -1;
        bool non_ref = false;
        for (uint32_t j = 0; j < nh; ++j) {
            non_ref |= !p.is_ref[h0 + j];  // regenerate_variation_events (:340), then trim_to (:416-424): never cleared
            if (smaller[j] == TRIM_NONE || rep[j] != j) continue;
            ++n_out;
            if (p.is_ref[h0 + j] && (ref_at < 0 || smaller[j] >= top)) top = smaller[j], ref_at = (int32_t)j;  // the last in the map's order (:411-413)
        }
        if (ref_at >= 0) {
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nh; ++j) rank += smaller[j] != TRIM_NONE && rep[j] == j && smaller[j] < smaller[ref_at];
            ref_at = (int32_t)rank;
        }
        p.region_n_out[g] = n_out;
        p.out_region_ref_hap[g] = ref_at;
        p.variation[g] = TRIM_VARIATION_SPAN | (non_ref ? TRIM_VARIATION_SET : 0);
    }
}

// ---- prefix sums ----------------------------------------------------------------------------------------------------------------
// in[0, n) -> exclusive sums out[0, n], by one workgroup of TRIM_SCAN_THREADS; the total to every thread
__device__ uint32_t trim_block_scan(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *sums) {
    const uint32_t t = threadIdx.x, chunk = (n + TRIM_SCAN_THREADS - 1) / TRIM_SCAN_THREADS;
    const uint32_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += in[i];
    __syncthreads();
    sums[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < TRIM_SCAN_THREADS; ++i) {
            const uint32_t v = sums[i];
            sums[i] = run;
            run += v;
        }
        sums[TRIM_SCAN_THREADS] = run;
    }
    __syncthreads();
    uint32_t run = sums[t];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = in[i];
        out[i] = run;
        run += v;
    }
    const uint32_t total = sums[TRIM_SCAN_THREADS];
    __syncthreads();
    if (t == 0) out[n] = total;
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(TRIM_SCAN_THREADS) void trim_scan_kernel(TrimParams p) {
    __shared__ uint32_t sums[TRIM_SCAN_THREADS + 1];
    const uint32_t t = threadIdx.x;
    const uint32_t n_out = trim_block_scan(p.region_n_out, p.out_region_hap_off, p.n_regions, sums);
    for (uint32_t h = t; h < p.n_haps; h += TRIM_SCAN_THREADS) {
        if (p.hap_fate[h] < 0) continue;
        const uint32_t o = p.out_region_hap_off[p.hap_region[h]] + (uint32_t)p.hap_fate[h];  // one representative per rank
        p.out_src[o] = h;
        p.out_len[o] = p.win_len[h];
        p.out_n_cigar[o] = p.new_n_cigar[h];
    }
    __syncthreads();
    trim_block_scan(p.out_len, p.out_hap_off, n_out, sums);
    trim_block_scan(p.out_n_cigar, p.out_cigar_off, n_out, sums);
}

__global__ __launch_bounds__(64) void trim_gather_kernel(TrimParams p) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x;
    if (o >= p.out_region_hap_off[p.n_regions]) return;
    const uint32_t h = p.out_src[o], n = p.out_len[o], nc = p.out_n_cigar[o];
    const uint8_t *src = p.hap_bases + p.hap_off[h] + p.win_first[h];
    uint8_t *dst = p.out_bases + p.out_hap_off[o];
    for (uint32_t i = lane; i < n; i += 64) dst[i] = upper(src[i]);  // ByteArrayAllele::new (byte_array_allele.rs:76)
    const uint32_t *cs = p.ws_cigar_b + p.cigar_off[h];
    uint32_t *cd = p.out_cigar + p.out_cigar_off[o];
    for (uint32_t i = lane; i < nc; i += 64) cd[i] = cs[i];
    if (lane == 0) {
        p.out_start[o] = p.new_start[h];
        p.out_source[o] = h - p.region_hap_off[p.hap_region[h]];
        p.out_is_ref[o] = p.is_ref[h] ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_trim(const EventsParams &e, const TrimParams &p, hipStream_t stream) {
    if (!p.n_regions) return hipSuccess;
    const hipError_t st = launch_event_maps(e, stream);
    if (st != hipSuccess) return st;
    trim_span_kernel<<<p.n_regions, 64, 0, stream>>>(p);
    if (p.n_haps) trim_hap_kernel<<<(p.n_haps + 63) / 64, 64, 0, stream>>>(p);
    if (p.n_haps) trim_rank_kernel<<<p.n_haps, 64, 0, stream>>>(p);
    trim_order_kernel<<<p.n_regions, TRIM_RANK_THREADS, 0, stream>>>(p);
    trim_scan_kernel<<<1, TRIM_SCAN_THREADS, 0, stream>>>(p);
    if (p.n_haps) trim_gather_kernel<<<p.n_haps, 64, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace phmm
