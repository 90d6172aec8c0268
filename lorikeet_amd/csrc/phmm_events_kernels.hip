// Event discovery for gfx950 (phmm_discover_events, include/phmm.h): the head of the reference's assign_genotype_likelihoods --
// the event map of every haplotype, the loci, the merged alleles of every locus and the haplotype -> allele map.  Integer and
// byte work only; no floating point in this file.
//
//   events_hap_kernel     one wave per haplotype walks the CIGAR (EventMap::process_cigar_for_initial_events, add_vc,
//                         make_block): 64 bases of an M block are compared at once, a ballot gives the mismatch offsets;
//                         MNP grouping and the same-start merge touch only the newest event, which stays in registers
//   events_region_kernel  one wave per region: the start positions inside the window as a bitmap in LDS, popcount prefix
//                         sums give the loci in ascending order; the region's status is that of its first failing haplotype
//   events_locus_kernel   one wave per locus, twice: first it counts (alleles, allele bytes), then -- behind the prefix sums of
//                         events_scan_kernel -- it writes.  get_overlapping_events per haplotype (lanes over haplotypes), the
//                         first-seen dedup, simple_merge's allele set, create_allele_mapper (lanes over haplotypes)
//   events_scan_kernel    one workgroup: exclusive prefix sums over regions / loci / haplotypes
//   events_hap_out_kernel the per-haplotype event maps, dense
// Nothing is appended through an atomic counter: every position comes from a prefix sum, so the output does not depend on
// scheduling.  The only atomics are order-free (bits of an LDS bitmap, a minimum).
#include "phmm_events_internal.hpp"

namespace phmm {

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4, OP_EQ = 7, OP_X = 8;

__device__ __forceinline__ bool regular(uint8_t b) {  // rust-bio's dna::alphabet(): "ACGTacgt"
    return b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'a' || b == 'c' || b == 'g' || b == 't';
}
__device__ __forceinline__ uint8_t upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }
__device__ __forceinline__ uint32_t type_of(uint32_t ref_len, uint32_t alt_len) {
    return ref_len == alt_len ? (alt_len == 1 ? EV_TYPE_SNP : EV_TYPE_MNP) : EV_TYPE_INDEL;
}

// ---- per haplotype ---------------------------------------------------------------------------------------------------------
struct HapWalk {
    const uint8_t *ref, *hap;
    HapEvent *evs;
    uint8_t *alt;
    uint32_t cap, lane;           // room of evs and of alt
    uint32_t n_ev = 0, n_alt = 0, collapsed = 0;
    bool block_failed = false;
    HapEvent cur{};               // evs[n_ev - 1]
    uint8_t cur_first = 0;        // ... and the first byte of its alt

    __device__ void append_alt(bool with_first, uint8_t first, const uint8_t *rest, uint32_t rest_len) {
        if (with_first) {
            if (lane == 0 && n_alt < cap) alt[n_alt] = first;
            ++n_alt;
        }
        for (uint32_t i = lane; i < rest_len; i += 64)
            if (n_alt + i < cap) alt[n_alt + i] = upper(rest[i]);
        n_alt += rest_len;
    }
    __device__ void store_cur() {
        if (lane == 0 && n_ev - 1 < cap) evs[n_ev - 1] = cur;
    }
    // a proposed event: [start, end], ref_len reference bases, the alt = `first` + rest_len haplotype bases from `rest`
    __device__ void propose(uint32_t start, uint32_t end, uint32_t ref_len, uint32_t type, uint8_t first, const uint8_t *rest,
                            uint32_t rest_len) {
        if (block_failed) return;
        const uint32_t alt_len = 1 + rest_len;
        if (!n_ev || cur.start != start) {  // add_vc: a new key
            cur = HapEvent{start, end, ref_len, n_alt, alt_len, type};
            cur_first = first;
            append_alt(true, first, rest, rest_len);
            ++n_ev;
            collapsed += type == EV_TYPE_NONE;
            store_cur();
            return;
        }
        // make_block(cur, proposal)
        const uint8_t cur_alt0 = cur_first, ref0 = upper(ref[start]);
        const bool cur_simple = cur.type == EV_TYPE_INDEL && ref0 == cur_alt0 && (cur.ref_len == 1 || cur.alt_len == 1);
        const bool new_simple = type == EV_TYPE_INDEL && ref0 == first && (ref_len == 1 || alt_len == 1);
        bool ok = cur.type != EV_TYPE_NONE;  // is_biallelic
        if (cur.type != EV_TYPE_SNP)
            ok = ok && ((cur_simple && cur.alt_len == 1 && new_simple && ref_len == 1) || (cur_simple && cur.ref_len == 1 && new_simple && alt_len == 1));
        else
            ok = ok && type != EV_TYPE_SNP;
        if (!ok) {
            block_failed = true;
            return;
        }
        const uint32_t block_type = type_of(cur.ref_len, cur.alt_len);  // get_type() on the copy of vc1, before the alleles change
        if (cur.type == EV_TYPE_SNP) {
            if (cur.ref_len == ref_len) {  // equal references: an insertion, the alt grows
                append_alt(false, 0, rest, rest_len);
                cur.alt_len += rest_len;
            } else {  // a deletion: its reference and end
                cur.ref_len = ref_len;
                cur.end = end;
            }
        } else if (cur.ref_len == 1) {  // insertion, then deletion
            cur.ref_len = ref_len;
            cur.end = end;
        } else {  // deletion, then insertion: the insertion's alt (cur's bytes are the pool's last)
            n_alt = cur.alt_off;
            append_alt(true, first, rest, rest_len);
            cur_first = first;
            cur.alt_len = alt_len;
        }
        cur.type = block_type;
        store_cur();
    }
};

__global__ __launch_bounds__(64) void events_hap_kernel(EventsParams p) {
    const uint32_t h = blockIdx.x, lane = threadIdx.x, g = p.hap_region[h];
    const uint8_t *ref = p.ref_bases + p.ref_off[g];
    const uint64_t ref_len = p.ref_off[g + 1] - p.ref_off[g], hap_len = p.hap_off[h + 1] - p.hap_off[h];
    const uint8_t *hap = p.hap_bases + p.hap_off[h];
    const uint32_t *cig = p.cigar + p.cigar_off[h], n_cig = p.cigar_off[h + 1] - p.cigar_off[h];
    HapWalk w;
    w.ref = ref;
    w.hap = hap;
    w.evs = p.ws_ev + p.ws_ev_off[h];
    w.alt = p.ws_alt + p.ws_ev_off[h];
    w.cap = p.ws_ev_off[h + 1] - p.ws_ev_off[h];
    w.lane = lane;
    uint64_t ref_pos = p.hap_start[h], ap = 0;
    int32_t status = 0;
    for (uint32_t ci = 0; ci < n_cig && !status; ++ci) {
        const uint32_t op = cig[ci] & 15u;
        const uint64_t len = cig[ci] >> 4;
        if (op == OP_I) {
            if (ref_pos > 0) {
                if (ref_pos - 1 >= ref_len) {
                    status = EV_CIGAR_OVERRUN;
                    break;
                }
                const uint8_t rb = ref[ref_pos - 1];
                if (!(ci == 0 || ci == n_cig - 1)) {
                    if (ap + len > hap_len) {
                        status = EV_CIGAR_OVERRUN;
                        break;
                    }
                    bool bad = false;
                    for (uint64_t i = lane; i < len; i += 64) bad |= !regular(hap[ap + i]);
                    if (regular(rb) && !__any(bad))
                        w.propose((uint32_t)ref_pos - 1, (uint32_t)ref_pos - 1, 1, EV_TYPE_INDEL, upper(rb), hap + ap, (uint32_t)len);
                }
            }
            ap += len;
        } else if (op == OP_S) {
            ap += len;
        } else if (op == OP_D) {
            if (ref_pos > 0) {
                if (ref_pos + len > ref_len) {
                    status = EV_CIGAR_OVERRUN;
                    break;
                }
                bool bad = false;
                for (uint64_t i = lane; i <= len; i += 64) bad |= !regular(ref[ref_pos - 1 + i]);
                if (!__any(bad))
                    w.propose((uint32_t)ref_pos - 1, (uint32_t)(ref_pos - 1 + len), (uint32_t)len + 1, EV_TYPE_INDEL, upper(ref[ref_pos - 1]), hap, 0);
            }
            ref_pos += len;
        } else if (op == OP_M || op == OP_EQ || op == OP_X) {
            if (ref_pos + len > ref_len || ap + len > hap_len) {
                status = EV_CIGAR_OVERRUN;
                break;
            }
            bool run = false;
            uint64_t run_start = 0, run_end = 0;
            auto emit = [&]() {
                const uint32_t n = (uint32_t)(run_end - run_start + 1);
                bool differs = false;  // ByteArrayAllele::new upper-cases: equal alleles collapse into one
                for (uint32_t i = lane; i < n; i += 64) differs |= upper(ref[ref_pos + run_start + i]) != upper(hap[ap + run_start + i]);
                const uint32_t type = __any(differs) ? (n == 1 ? EV_TYPE_SNP : EV_TYPE_MNP) : EV_TYPE_NONE;
                w.propose((uint32_t)(ref_pos + run_start), (uint32_t)(ref_pos + run_end), n, type, upper(hap[ap + run_start]),
                          hap + ap + run_start + 1, n - 1);
            };
            for (uint64_t c = 0; c < len; c += 64) {
                const uint64_t o = c + lane;
                bool mis = false;
                if (o < len) {
                    const uint8_t r = ref[ref_pos + o], a = hap[ap + o];
                    mis = r != a && regular(r) && regular(a);
                }
                unsigned long long mask = __ballot(mis);
                while (mask) {
                    const uint64_t off = c + (uint64_t)__builtin_ctzll(mask);
                    mask &= mask - 1;
                    if (run && off - run_end <= (uint64_t)p.dist) {
                        run_end = off;
                    } else {
                        if (run) emit();
                        run = true;
                        run_start = run_end = off;
                    }
                }
            }
            if (run) emit();
            ref_pos += len;
            ap += len;
        } else {
            status = EV_BAD_OPERATOR;
        }
    }
    if (!status) status = w.block_failed ? EV_BLOCK : w.collapsed ? EV_ALLELES : 0;
    if (lane == 0) {
        p.hap_n_ev[h] = status ? 0 : w.n_ev;
        p.hap_n_alt[h] = status ? 0 : w.n_alt;
        p.hap_status[h] = status;
    }
}

// ---- per region: the loci -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void events_region_kernel(EventsParams p) {
    __shared__ uint32_t bits[EV_MAX_REF / 32], pref[EV_MAX_REF / 32 + 1];
    __shared__ uint32_t first_bad;
    const uint32_t g = blockIdx.x, lane = threadIdx.x;
    const uint32_t h0 = p.region_hap_off[g], h1 = p.region_hap_off[g + 1], ref_len = p.ref_off[g + 1] - p.ref_off[g];
    const uint32_t n_words = (ref_len + 31) / 32;
    for (uint32_t w = lane; w < n_words; w += 64) bits[w] = 0;
    if (lane == 0) first_bad = NONE;
    __syncthreads();
    for (uint32_t h = h0 + lane; h < h1; h += 64)
        if (p.hap_status[h] < 0) atomicMin(&first_bad, h);
    __syncthreads();
    if (first_bad != NONE) {
        if (lane == 0) {
            p.region_status[g] = p.hap_status[first_bad];
            p.region_n_loci[g] = 0;
        }
        return;
    }
    const uint64_t rs = p.ref_start[g], ws = p.win_start[g], we = p.win_end[g];
    for (uint32_t h = h0; h < h1; ++h) {
        const HapEvent *evs = p.ws_ev + p.ws_ev_off[h];
        for (uint32_t k = lane; k < p.hap_n_ev[h]; k += 64) {
            const uint32_t s = evs[k].start;
            if (s < ref_len && rs + s >= ws && rs + s <= we) atomicOr(&bits[s >> 5], 1u << (s & 31));
        }
    }
    __syncthreads();
    if (lane == 0) {
        uint32_t n = 0;
        for (uint32_t w = 0; w < n_words; ++w) {
            pref[w] = n;
            n += __popc(bits[w]);
        }
        pref[n_words] = n;
        p.region_status[g] = 0;
        p.region_n_loci[g] = n;
    }
    __syncthreads();
    uint32_t *loci = p.loci + p.ref_off[g];
    for (uint32_t w = lane; w < n_words; w += 64) {
        uint32_t m = bits[w], at = pref[w];
        while (m) {
            loci[at++] = w * 32 + (uint32_t)__builtin_ctz(m);
            m &= m - 1;
        }
    }
}

// ---- prefix sums ----------------------------------------------------------------------------------------------------------------
// in[0, n) -> exclusive sums out[0, n], by one workgroup of EV_SCAN_THREADS; `in` and `out` may be the same array when out
// has room for n + 1.  Returns the total to every thread.
__device__ uint32_t block_scan(const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *sums) {
    const uint32_t t = threadIdx.x, chunk = (n + EV_SCAN_THREADS - 1) / EV_SCAN_THREADS;
    const uint32_t lo = min(n, t * chunk), hi = min(n, lo + chunk);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += in[i];
    __syncthreads();
    sums[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < EV_SCAN_THREADS; ++i) {
            const uint32_t v = sums[i];
            sums[i] = run;
            run += v;
        }
        sums[EV_SCAN_THREADS] = run;
    }
    __syncthreads();
    uint32_t run = sums[t];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = in[i];
        out[i] = run;
        run += v;
    }
    const uint32_t total = sums[EV_SCAN_THREADS];
    __syncthreads();
    if (t == 0) out[n] = total;
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(EV_SCAN_THREADS) void events_scan_regions_kernel(EventsParams p) {
    __shared__ uint32_t sums[EV_SCAN_THREADS + 1];
    block_scan(p.region_n_loci, p.locus_base, p.n_regions, sums);
}

__global__ __launch_bounds__(EV_SCAN_THREADS) void events_scan_kernel(EventsParams p) {
    __shared__ uint32_t sums[EV_SCAN_THREADS + 1];
    const uint32_t t = threadIdx.x, n_loci = p.locus_base[p.n_regions];
    // a region that failed at one of its loci (simple_merge) has no events
    for (uint32_t g = t; g < p.n_regions; g += EV_SCAN_THREADS)
        if (p.region_status[g] < 0)
            for (uint32_t l = p.locus_base[g]; l < p.locus_base[g + 1]; ++l)
                for (uint32_t k = 0; k < 4; ++k) p.locus_cnt[k * p.max_loci + l] = 0;
    __syncthreads();
    for (uint32_t k = 0; k < 4; ++k) {
        uint32_t *c = p.locus_cnt + (size_t)k * p.max_loci;
        const uint32_t total = block_scan(c, c, n_loci, sums);
        if (t == 0) p.required[k] = total;
    }
    for (uint32_t g = t; g <= p.n_regions; g += EV_SCAN_THREADS) p.region_event_off[g] = p.locus_cnt[p.locus_base[g]];
    // the haplotypes' own events, dense: none for a failed region
    for (uint32_t h = t; h < p.n_haps; h += EV_SCAN_THREADS)
        if (p.region_status[p.hap_region[h]] < 0) p.hap_n_ev[h] = p.hap_n_alt[h] = 0;
    __syncthreads();
    uint32_t total = block_scan(p.hap_n_ev, p.hap_dense_ev, p.n_haps, sums);
    if (t == 0) p.required[4] = total;
    total = block_scan(p.hap_n_alt, p.hap_dense_alt, p.n_haps, sums);
    if (t == 0) p.required[5] = total;
}

__device__ __forceinline__ bool fits(const EventsParams &p, uint32_t first, uint32_t last) {
    for (uint32_t k = first; k < last; ++k)
        if (p.required[k] > p.cap[k]) return false;
    return true;
}

__global__ __launch_bounds__(64) void events_hap_out_kernel(EventsParams p) {
    if (!p.hap_event_start || !fits(p, 4, 6)) return;
    const uint32_t h = blockIdx.x, lane = threadIdx.x, g = p.hap_region[h];
    const uint32_t e0 = p.hap_dense_ev[h], b0 = p.hap_dense_alt[h], slot = p.ws_ev_off[h];
    const HapEvent *evs = p.ws_ev + slot;
    const int64_t rs = (int64_t)p.ref_start[g];
    for (uint32_t k = lane; k < p.hap_n_ev[h]; k += 64) {
        p.hap_event_start[e0 + k] = rs + evs[k].start;
        p.hap_event_end[e0 + k] = rs + evs[k].end;
        p.hap_event_ref_length[e0 + k] = evs[k].ref_len;
        p.hap_event_alt_off[e0 + k] = b0 + evs[k].alt_off;
        p.hap_event_type[e0 + k] = evs[k].type;
    }
    for (uint32_t i = lane; i < p.hap_n_alt[h]; i += 64) p.hap_event_alt[b0 + i] = p.ws_alt[slot + i];
}

// ---- per locus ------------------------------------------------------------------------------------------------------------------
// An allele of the merged context: the reference (ev == nullptr, star false), '*', or the alt of an event extended by the
// reference's tail behind the event's own reference allele.
struct AlleleView {
    const uint8_t *ref_at_loc;   // the region's reference from the locus on
    uint32_t merged_ref_len;
    __device__ uint32_t length(const HapEvent *ev, bool star) const {
        return star ? 1 : ev ? ev->alt_len + (merged_ref_len - ev->ref_len) : merged_ref_len;
    }
    __device__ uint8_t byte(const HapEvent *ev, const uint8_t *pool, bool star, uint32_t i) const {
        if (star) return '*';
        if (!ev) return upper(ref_at_loc[i]);
        return i < ev->alt_len ? pool[ev->alt_off + i] : upper(ref_at_loc[ev->ref_len + (i - ev->alt_len)]);
    }
    __device__ bool equal(const HapEvent *a, const uint8_t *pa, bool sa, const HapEvent *b, const uint8_t *pb, bool sb) const {
        const uint32_t n = length(a, sa);
        if (n != length(b, sb)) return false;
        for (uint32_t i = 0; i < n; ++i)
            if (byte(a, pa, sa, i) != byte(b, pb, sb, i)) return false;
        return true;
    }
};

template <bool WRITE>
__global__ __launch_bounds__(64) void events_locus_kernel(EventsParams p) {
    __shared__ uint32_t ov[EV_MAX_HAPS * EV_OVERLAP];       // per haplotype: its overlapping events (index in its slot) or NONE
    __shared__ uint32_t uq_ev[EV_MAX_HAPS * EV_OVERLAP];    // the unique events at the locus: slot index of the event ...
    __shared__ uint16_t uq_h[EV_MAX_HAPS * EV_OVERLAP];     // ... and its haplotype inside the region
    __shared__ uint32_t al[EV_MAX_HAPS * EV_OVERLAP];       // the alt alleles in first-seen order: index into uq_*
    const uint32_t lane = threadIdx.x, n_loci = p.locus_base[p.n_regions];
    if (WRITE && !fits(p, 0, 4)) return;
    for (uint32_t L = blockIdx.x; L < n_loci; L += gridDim.x) {
        __syncthreads();
        uint32_t lo = 0, hi = p.n_regions;  // the region: the last g with locus_base[g] <= L
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (p.locus_base[mid] <= L) lo = mid;
            else hi = mid;
        }
        const uint32_t g = lo;
        if (WRITE && p.region_status[g] < 0) continue;
        const uint32_t loc = p.loci[p.ref_off[g] + (L - p.locus_base[g])];
        const uint32_t h0 = p.region_hap_off[g], nh = p.region_hap_off[g + 1] - h0;
        const uint8_t *ref = p.ref_bases + p.ref_off[g];
        // -- get_overlapping_events per haplotype
        for (uint32_t hl = lane; hl < nh; hl += 64) {
            const HapEvent *evs = p.ws_ev + p.ws_ev_off[h0 + hl];
            uint32_t a = 0, b = p.hap_n_ev[h0 + hl];  // j = events with start <= loc
            while (a < b) {
                const uint32_t mid = (a + b) / 2;
                if (evs[mid].start <= loc) a = mid + 1;
                else b = mid;
            }
            uint32_t cand[EV_OVERLAP], n = 0;
            bool has_ins = false;
            uint32_t del = NONE;
            for (uint32_t k = a > EV_OVERLAP ? a - EV_OVERLAP : 0; k < a; ++k) {
                const HapEvent e = evs[k];
                if (e.end < loc) continue;
                has_ins |= e.type == EV_TYPE_INDEL && e.ref_len == 1;
                if (del == NONE && e.type == EV_TYPE_INDEL && e.alt_len == 1 && e.end == loc) del = k;
                cand[n++] = k;
            }
            uint32_t m = 0;
            for (uint32_t i = 0; i < EV_OVERLAP; ++i) {
                uint32_t v = NONE;
                while (m < n && v == NONE) {
                    if (!(has_ins && cand[m] == del)) v = cand[m];  // the deletion ending here gives way to the insertion
                    ++m;
                }
                ov[hl * EV_OVERLAP + i] = v;
            }
        }
        __syncthreads();
        // -- get_variant_contexts_from_active_haplotypes: the first occurrence in haplotype order by (start, alleles)
        uint32_t nu = 0;
        for (uint32_t hl = 0; hl < nh; ++hl) {
            const uint32_t slot = p.ws_ev_off[h0 + hl];
            for (uint32_t i = 0; i < EV_OVERLAP; ++i) {
                const uint32_t k = ov[hl * EV_OVERLAP + i];
                if (k == NONE) continue;
                const HapEvent e = p.ws_ev[slot + k];
                if (!p.spanning && e.start != loc) continue;
                bool same = false;
                for (uint32_t u = lane; u < nu && !same; u += 64) {
                    const uint32_t us = p.ws_ev_off[h0 + uq_h[u]];
                    const HapEvent o = p.ws_ev[us + uq_ev[u]];
                    if (o.start != e.start || o.ref_len != e.ref_len || o.alt_len != e.alt_len) continue;
                    same = true;
                    for (uint32_t j = 0; j < e.alt_len && same; ++j) same = p.ws_alt[us + o.alt_off + j] == p.ws_alt[slot + e.alt_off + j];
                }
                if (!__any(same)) {
                    if (lane == 0) {
                        uq_ev[nu] = k;
                        uq_h[nu] = (uint16_t)hl;
                    }
                    ++nu;
                    __syncthreads();
                }
            }
        }
        uint32_t *cnt = p.locus_cnt + L;
        if (!nu) {  // make_merged_variant_context: None
            if (!WRITE && lane == 0)
                for (uint32_t k = 0; k < 4; ++k) cnt[(size_t)k * p.max_loci] = 0;
            continue;
        }
        // -- simple_merge: the longest reference, the span of the first longest context, the alleles in first-seen order.
        //    An event that starts before the locus has become (reference base, '*') (replace_span_dels).
        uint32_t merged_ref_len = 0, vc_end = loc;
        for (uint32_t u = 0; u < nu; ++u) {
            const HapEvent e = p.ws_ev[p.ws_ev_off[h0 + uq_h[u]] + uq_ev[u]];
            const bool span = e.start != loc;
            merged_ref_len = max(merged_ref_len, span ? 1u : e.ref_len);
            if (!span && e.end > vc_end) vc_end = e.end;
        }
        const AlleleView V{ref + loc, merged_ref_len};
        uint32_t na = 0, n_bytes = merged_ref_len, star_at = NONE;
        bool ref_in = false, lost_ref = false;
        for (uint32_t u = 0; u < nu; ++u) {
            const uint32_t us = p.ws_ev_off[h0 + uq_h[u]];
            const HapEvent *e = p.ws_ev + us + uq_ev[u];
            const bool span = e->start != loc;
            const bool ref_first = (span ? 1u : e->ref_len) == merged_ref_len;
            for (int step = 0; step < 2; ++step) {
                const bool is_ref = (step == 0) == ref_first;
                // is it in the set already?  (bases alone: ByteArrayAllele's equality)
                bool same = false;
                for (uint32_t a = lane; a < na + 1 && !same; a += 64) {
                    const HapEvent *oe = nullptr;
                    const uint8_t *op = nullptr;
                    bool ostar = false;
                    if (a == na) {
                        if (!ref_in) continue;
                    } else {
                        const uint32_t os = p.ws_ev_off[h0 + uq_h[al[a]]];
                        oe = p.ws_ev + os + uq_ev[al[a]];
                        op = p.ws_alt + os;
                        ostar = oe->start != loc;
                    }
                    same = V.equal(is_ref ? nullptr : e, p.ws_alt + us, !is_ref && span, oe, op, ostar);
                }
                if (__any(same)) continue;
                if (is_ref) {
                    ref_in = true;
                } else {
                    if (span) star_at = na;
                    if (lane == 0) al[na] = u;
                    n_bytes += V.length(e, span);
                    ++na;
                    __syncthreads();
                }
            }
            lost_ref |= !ref_in;  // its bases are in the set as an alt: make_alleles finds no reference allele
        }
        if (lost_ref) {
            if (!WRITE && lane == 0) {
                atomicMin(&p.region_status[g], EV_MERGE);
                for (uint32_t k = 0; k < 4; ++k) cnt[(size_t)k * p.max_loci] = 0;
            }
            continue;
        }
        if (!WRITE) {
            if (lane == 0) {
                cnt[0] = 1;
                cnt[(size_t)p.max_loci] = na + 1;
                cnt[(size_t)2 * p.max_loci] = n_bytes;
                cnt[(size_t)3 * p.max_loci] = nh;
            }
            continue;
        }
        const uint32_t e_at = cnt[0], a_at = cnt[(size_t)p.max_loci], b_at = cnt[(size_t)2 * p.max_loci], m_at = cnt[(size_t)3 * p.max_loci];
        // -- create_allele_mapper, lanes over haplotypes
        for (uint32_t hl = lane; hl < nh; hl += 64) {
            const uint32_t slot = p.ws_ev_off[h0 + hl];
            int32_t res = ov[hl * EV_OVERLAP] == NONE ? 0 : -1;
            for (uint32_t i = 0; i < EV_OVERLAP; ++i) {
                const uint32_t k = ov[hl * EV_OVERLAP + i];
                if (k == NONE) break;
                const HapEvent *e = p.ws_ev + slot + k;
                int32_t idx = -1;
                if (e->start == loc) {
                    if (e->ref_len > merged_ref_len) continue;
                    if (V.equal(e, p.ws_alt + slot, false, nullptr, nullptr, false)) idx = 0;
                    for (uint32_t a = 0; a < na && idx < 0; ++a) {
                        const uint32_t os = p.ws_ev_off[h0 + uq_h[al[a]]];
                        const HapEvent *oe = p.ws_ev + os + uq_ev[al[a]];
                        if (V.equal(e, p.ws_alt + slot, false, oe, p.ws_alt + os, oe->start != loc)) idx = (int32_t)a + 1;
                    }
                    if (idx < 0) continue;
                } else {
                    idx = p.spanning && star_at != NONE ? (int32_t)star_at + 1 : 0;
                }
                // The first list the reference pushes the haplotype to.  It stops at an event that started earlier, which is the
                // first one it meets, and a map holds one event per start: there is no second list (PHMM_EV_HAP_IN_TWO_ALLELES).
                res = idx;
                break;
            }
            p.event_hap_allele[m_at + hl] = res;
        }
        __syncthreads();
        // -- the event and its alleles
        if (lane == 0) {
            const uint64_t rs = p.ref_start[g], vs = rs + loc, ve = rs + vc_end;
            p.event_region[e_at] = g;
            p.event_allele_off[e_at] = a_at;
            p.event_loc[e_at] = (int64_t)vs;
            p.vc_start[e_at] = (int64_t)vs;
            p.vc_end[e_at] = (int64_t)ve;
            p.event_start[e_at] = (int64_t)(vs < p.margin ? 0 : vs - p.margin);  // expand_within_contig
            p.event_end[e_at] = (int64_t)min(p.contig_len[g], ve + p.margin);
            p.event_flags[e_at] = 0;
        }
        uint32_t at = b_at;
        for (uint32_t a = 0; a <= na; ++a) {  // the reference first
            const HapEvent *e = nullptr;
            const uint8_t *pool = nullptr;
            bool star = false;
            if (a) {
                const uint32_t os = p.ws_ev_off[h0 + uq_h[al[a - 1]]];
                e = p.ws_ev + os + uq_ev[al[a - 1]];
                pool = p.ws_alt + os;
                star = e->start != loc;
            }
            const uint32_t n = V.length(e, star);
            if (lane == 0) {
                p.allele_length[a_at + a] = n;
                p.allele_kind[a_at + a] = star ? 1 : 0;
                p.allele_bases_off[a_at + a] = at;
            }
            for (uint32_t i = lane; i < n; i += 64) p.allele_bases[at + i] = V.byte(e, pool, star, i);
            at += n;
        }
    }
}

}  // namespace

hipError_t launch_events(const EventsParams &p, hipStream_t stream) {
    if (!p.n_regions) return hipSuccess;
    const uint32_t locus_blocks = p.max_loci < 2048 ? p.max_loci : 2048;  // max_loci: the host's bound on the loci, at least 1
    if (p.n_haps) events_hap_kernel<<<p.n_haps, 64, 0, stream>>>(p);
    events_region_kernel<<<p.n_regions, 64, 0, stream>>>(p);
    events_scan_regions_kernel<<<1, EV_SCAN_THREADS, 0, stream>>>(p);
    events_locus_kernel<false><<<locus_blocks, 64, 0, stream>>>(p);
    events_scan_kernel<<<1, EV_SCAN_THREADS, 0, stream>>>(p);
    events_locus_kernel<true><<<locus_blocks, 64, 0, stream>>>(p);
    if (p.n_haps) events_hap_out_kernel<<<p.n_haps, 64, 0, stream>>>(p);
    return hipGetLastError();
}

// events_hap_kernel alone (phmm_trim_regions): every haplotype's event map into the workspace -- ws_ev / ws_alt by ws_ev_off,
// hap_n_ev, hap_n_alt, hap_status -- and nothing else of EventsParams is read or written.
hipError_t launch_event_maps(const EventsParams &p, hipStream_t stream) {
    if (p.n_haps) events_hap_kernel<<<p.n_haps, 64, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace phmm
