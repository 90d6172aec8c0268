// phmm_discover_events (include/phmm.h): host side -- validation, the workspace bounds, staging.  The events are found on the
// device (phmm_events_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "phmm_events_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_discover_events: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

// ByteArrayAllele::acceptable_allele_bases (src/model/byte_array_allele.rs:182-207) minus the symbolic and '*' forms
bool accepted(uint8_t b) {
    static const char ok[] = "ACGTNacgtnRYKMSWBDHVU";
    return b && strchr(ok, (int)b);
}

}  // namespace

extern "C" {

int phmm_discover_events(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                         const uint64_t *region_ref_start, const uint64_t *region_window_start, const uint64_t *region_window_end,
                         const uint64_t *region_contig_length, const uint32_t *region_hap_off, const uint32_t *hap_off,
                         const uint8_t *hap_bases, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                         const uint32_t *hap_start_wrt_ref, uint32_t max_mnp_distance, int include_spanning_events,
                         uint32_t overlap_margin, const uint32_t *capacity, uint32_t *required, uint32_t *region_event_off,
                         int32_t *region_status, uint32_t *event_region, uint32_t *event_allele_off, int64_t *event_start,
                         int64_t *event_end, int64_t *event_loc, int64_t *vc_start, int64_t *vc_end, uint32_t *event_flags,
                         int32_t *event_hap_allele, uint32_t *allele_length, uint8_t *allele_kind, uint32_t *allele_bases_off,
                         uint8_t *allele_bases, uint32_t *hap_event_off, int64_t *hap_event_start, int64_t *hap_event_end,
                         uint32_t *hap_event_ref_length, uint32_t *hap_event_alt_off, uint8_t *hap_event_alt,
                         uint32_t *hap_event_type) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!capacity || !required || !region_event_off) return fail(h, "null array");
        const bool maps = hap_event_off != nullptr;
        if (maps && (!hap_event_start || !hap_event_end || !hap_event_ref_length || !hap_event_alt_off || !hap_event_alt || !hap_event_type))
            return fail(h, "null array (the per-haplotype event maps come together)");
        if (!n_regions) {
            std::fill(required, required + 6, 0u);
            region_event_off[0] = 0;
            event_allele_off ? (void)(event_allele_off[0] = 0) : (void)0;
            allele_bases_off ? (void)(allele_bases_off[0] = 0) : (void)0;
            return PHMM_OK;
        }
        if (!region_ref_off || !region_ref_start || !region_window_start || !region_window_end || !region_contig_length ||
            !region_hap_off || !region_status || !event_region || !event_allele_off || !event_start || !event_end || !event_loc ||
            !vc_start || !vc_end || !event_flags || !allele_length || !allele_kind || !allele_bases_off)
            return fail(h, "null array");
        if (region_ref_off[0]) return fail(h, "region_ref_off does not start at 0");
        if (region_hap_off[0]) return fail(h, "region_hap_off does not start at 0");
        uint64_t work = 0, max_loci = 0;
        for (uint32_t g = 0; g < n_regions; ++g) {
            const std::string rg = "region " + std::to_string(g) + ": ";
            if (region_ref_off[g + 1] < region_ref_off[g]) return fail(h, rg + "region_ref_off not monotonic");
            if (region_hap_off[g + 1] < region_hap_off[g]) return fail(h, rg + "region_hap_off not monotonic");
            const uint32_t len = region_ref_off[g + 1] - region_ref_off[g], nh = region_hap_off[g + 1] - region_hap_off[g];
            if (len > EV_MAX_REF) return fail(h, rg + std::to_string(len) + " reference bases, more than " + std::to_string(EV_MAX_REF));
            if (nh > EV_MAX_HAPS) return fail(h, rg + std::to_string(nh) + " haplotypes, more than " + std::to_string(EV_MAX_HAPS));
            if (!region_contig_length[g]) return fail(h, rg + "contig length 0");
            if (region_ref_start[g] >> 62 || region_contig_length[g] >> 62) return fail(h, rg + "position beyond 2^62");
            max_loci += len;
        }
        const uint32_t n_ref = region_ref_off[n_regions], n_haps = region_hap_off[n_regions];
        if (n_ref && !ref_bases) return fail(h, "null array");
        if (n_haps && (!hap_off || !hap_cigar_off || !hap_start_wrt_ref || !event_hap_allele)) return fail(h, "null array");
        for (uint32_t i = 0; i < n_ref; ++i)
            if (!accepted(ref_bases[i])) return fail(h, "reference base " + std::to_string(i) + " is not a base the reference's alleles take");
        if (n_haps && hap_off[0]) return fail(h, "hap_off does not start at 0");
        if (n_haps && hap_cigar_off[0]) return fail(h, "hap_cigar_off does not start at 0");
        std::vector<uint32_t> slot(n_haps + 1, 0), hap_region(n_haps);
        for (uint32_t g = 0; g < n_regions; ++g)
            for (uint32_t k = region_hap_off[g]; k < region_hap_off[g + 1]; ++k) hap_region[k] = g;
        for (uint32_t k = 0; k < n_haps; ++k) {
            const std::string hp = "haplotype " + std::to_string(k) + ": ";
            if (hap_off[k + 1] < hap_off[k]) return fail(h, hp + "hap_off not monotonic");
            if (hap_cigar_off[k + 1] < hap_cigar_off[k]) return fail(h, hp + "hap_cigar_off not monotonic");
            // every event takes a CIGAR element or a haplotype base of its own, every alt byte too
            work += (uint64_t)(hap_off[k + 1] - hap_off[k]) + (hap_cigar_off[k + 1] - hap_cigar_off[k]) + 8;
            if (work >> 31) return fail(h, "haplotype bases + CIGAR elements + 8 per haplotype reach 2^31");
            slot[k + 1] = (uint32_t)work;
        }
        const uint32_t n_hap_bases = n_haps ? hap_off[n_haps] : 0, n_cigar = n_haps ? hap_cigar_off[n_haps] : 0;
        if ((n_hap_bases && !hap_bases) || (n_cigar && !hap_cigar)) return fail(h, "null array");
        for (uint32_t i = 0; i < n_hap_bases; ++i)
            if (!accepted(hap_bases[i])) return fail(h, "haplotype base " + std::to_string(i) + " is not a base the reference's alleles take");
        for (uint32_t i = 0; i < n_cigar; ++i)
            if ((hap_cigar[i] & 15u) > 8 || !(hap_cigar[i] >> 4))
                return fail(h, "CIGAR element " + std::to_string(i) + ": unknown operator or length 0");
        if ((capacity[1] && !allele_bases_off) || (capacity[2] && !allele_bases)) return fail(h, "null array");
        max_loci = std::min<uint64_t>(max_loci, work) + 1;

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->events_staging;
        hipStream_t S = h->streams[0];
        const uint32_t cap[6] = {capacity[0], capacity[1], capacity[2], capacity[3], maps ? capacity[4] : 0, maps ? capacity[5] : 0};
        StageLayout L;
        const auto s_ro = L.in(region_ref_off, n_regions + 1);
        const auto s_rb = L.in(ref_bases, n_ref);
        const auto s_rs = L.in(region_ref_start, n_regions), s_ws = L.in(region_window_start, n_regions), s_we = L.in(region_window_end, n_regions);
        const auto s_cl = L.in(region_contig_length, n_regions);
        const auto s_rh = L.in(region_hap_off, n_regions + 1), s_hr = L.in(hap_region.data(), n_haps);
        const auto s_ho = L.in(hap_off, n_haps ? n_haps + 1 : 0);
        const auto s_hb = L.in(hap_bases, n_hap_bases);
        const auto s_co = L.in(hap_cigar_off, n_haps ? n_haps + 1 : 0), s_cg = L.in(hap_cigar, n_cigar), s_hs = L.in(hap_start_wrt_ref, n_haps);
        const auto s_sl = L.in(slot.data(), n_haps + 1);
        L.end_inputs();
        // The haplotypes' event slots are sized for the worst case (25 bytes per haplotype base and CIGAR element) and never
        // copied: they lie in a device allocation of their own, so the pinned mirror does not pay for them.
        StageLayout D;
        const auto w_ev = D.scratch<HapEvent>(work);
        const auto w_al = D.scratch<uint8_t>(work);
        const auto w_lc = D.scratch<uint32_t>(4 * max_loci);
        const auto w_ne = L.scratch<uint32_t>(n_haps), w_na = L.scratch<uint32_t>(n_haps);
        const auto w_hs = L.scratch<int32_t>(n_haps);
        const auto w_lo = L.scratch<uint32_t>(n_ref), w_nl = L.scratch<uint32_t>(n_regions), w_lb = L.scratch<uint32_t>(n_regions + 1);
        const auto w_de = L.scratch<uint32_t>(n_haps + 1), w_da = L.scratch<uint32_t>(n_haps + 1);
        const auto o_rq = L.out<uint32_t>(6);
        const auto o_st = L.out<int32_t>(n_regions);
        const auto o_re = L.out<uint32_t>(n_regions + 1);
        const auto o_er = L.out<uint32_t>(cap[0]), o_ea = L.out<uint32_t>(cap[0]), o_ef = L.out<uint32_t>(cap[0]);
        const auto o_es = L.out<int64_t>(cap[0]), o_ee = L.out<int64_t>(cap[0]), o_el = L.out<int64_t>(cap[0]), o_vs = L.out<int64_t>(cap[0]),
                   o_ve = L.out<int64_t>(cap[0]);
        const auto o_hm = L.out<int32_t>(cap[3]);
        const auto o_al = L.out<uint32_t>(cap[1]), o_ao = L.out<uint32_t>(cap[1]);
        const auto o_ak = L.out<uint8_t>(cap[1]), o_ab = L.out<uint8_t>(cap[2]);
        const auto o_he = L.out<uint32_t>(maps ? n_haps + 1 : 0);
        const auto o_hS = L.out<int64_t>(cap[4]), o_hE = L.out<int64_t>(cap[4]);
        const auto o_hr = L.out<uint32_t>(cap[4]), o_ho = L.out<uint32_t>(cap[4]), o_ht = L.out<uint32_t>(cap[4]);
        const auto o_hb = L.out<uint8_t>(cap[5]);
        if (!h->events_scratch.reserve(h, D, "event discovery workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "event discovery staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;

        EventsParams p{};
        p.n_regions = n_regions;
        p.n_haps = n_haps;
        p.ref_off = W.dev_ptr(s_ro);
        p.ref_bases = W.dev_ptr(s_rb);
        p.ref_start = W.dev_ptr(s_rs);
        p.win_start = W.dev_ptr(s_ws);
        p.win_end = W.dev_ptr(s_we);
        p.contig_len = W.dev_ptr(s_cl);
        p.region_hap_off = W.dev_ptr(s_rh);
        p.hap_region = W.dev_ptr(s_hr);
        p.hap_off = W.dev_ptr(s_ho);
        p.hap_bases = W.dev_ptr(s_hb);
        p.cigar_off = W.dev_ptr(s_co);
        p.cigar = W.dev_ptr(s_cg);
        p.hap_start = W.dev_ptr(s_hs);
        p.dist = max_mnp_distance;
        p.spanning = include_spanning_events != 0;
        p.margin = overlap_margin;
        std::copy(cap, cap + 6, p.cap);
        p.max_loci = (uint32_t)max_loci;
        p.ws_ev_off = W.dev_ptr(s_sl);
        p.ws_ev = h->events_scratch.ptr(w_ev);
        p.ws_alt = h->events_scratch.ptr(w_al);
        p.hap_n_ev = W.dev_ptr(w_ne);
        p.hap_n_alt = W.dev_ptr(w_na);
        p.hap_status = W.dev_ptr(w_hs);
        p.loci = W.dev_ptr(w_lo);
        p.region_n_loci = W.dev_ptr(w_nl);
        p.locus_base = W.dev_ptr(w_lb);
        p.locus_cnt = h->events_scratch.ptr(w_lc);
        p.hap_dense_ev = maps ? W.dev_ptr(o_he) : W.dev_ptr(w_de);
        p.hap_dense_alt = W.dev_ptr(w_da);
        p.required = W.dev_ptr(o_rq);
        p.region_status = W.dev_ptr(o_st);
        p.region_event_off = W.dev_ptr(o_re);
        p.event_region = W.dev_ptr(o_er);
        p.event_allele_off = W.dev_ptr(o_ea);
        p.event_flags = W.dev_ptr(o_ef);
        p.event_start = W.dev_ptr(o_es);
        p.event_end = W.dev_ptr(o_ee);
        p.event_loc = W.dev_ptr(o_el);
        p.vc_start = W.dev_ptr(o_vs);
        p.vc_end = W.dev_ptr(o_ve);
        p.event_hap_allele = W.dev_ptr(o_hm);
        p.allele_length = W.dev_ptr(o_al);
        p.allele_bases_off = W.dev_ptr(o_ao);
        p.allele_kind = W.dev_ptr(o_ak);
        p.allele_bases = W.dev_ptr(o_ab);
        p.hap_event_start = maps ? W.dev_ptr(o_hS) : nullptr;
        p.hap_event_end = W.dev_ptr(o_hE);
        p.hap_event_ref_length = W.dev_ptr(o_hr);
        p.hap_event_alt_off = W.dev_ptr(o_ho);
        p.hap_event_type = W.dev_ptr(o_ht);
        p.hap_event_alt = W.dev_ptr(o_hb);
        if (!stage_round_trip(h, W, L, S, "event discovery", [&] { return hip_ok(h, launch_events(p, S), "phmm_events kernels"); })) return PHMM_ERR_HIP;
        const uint32_t *rq = W.host_ptr(o_rq);
        std::copy(rq, rq + 6, required);
        for (int k = 0; k < (maps ? 6 : 4); ++k)
            if (rq[k] > cap[k]) {
                if (!maps) required[4] = required[5] = 0;
                h->err = "phmm_discover_events: capacity " + std::to_string(k) + " is " + std::to_string(cap[k]) + ", " + std::to_string(rq[k]) + " needed";
                return h->err_code = PHMM_ERR_EVENT_CAPACITY;
            }
        if (!maps) required[4] = required[5] = 0;
        const size_t ne = rq[0], na = rq[1], nb = rq[2], nm = rq[3];
        memcpy(region_status, W.host_ptr(o_st), 4 * (size_t)n_regions);
        memcpy(region_event_off, W.host_ptr(o_re), 4 * ((size_t)n_regions + 1));
        if (ne) {
            memcpy(event_region, W.host_ptr(o_er), 4 * ne);
            memcpy(event_allele_off, W.host_ptr(o_ea), 4 * ne);
            memcpy(event_flags, W.host_ptr(o_ef), 4 * ne);
            memcpy(event_start, W.host_ptr(o_es), 8 * ne);
            memcpy(event_end, W.host_ptr(o_ee), 8 * ne);
            memcpy(event_loc, W.host_ptr(o_el), 8 * ne);
            memcpy(vc_start, W.host_ptr(o_vs), 8 * ne);
            memcpy(vc_end, W.host_ptr(o_ve), 8 * ne);
        }
        event_allele_off[ne] = (uint32_t)na;
        if (nm) memcpy(event_hap_allele, W.host_ptr(o_hm), 4 * nm);
        if (na) {
            memcpy(allele_length, W.host_ptr(o_al), 4 * na);
            memcpy(allele_bases_off, W.host_ptr(o_ao), 4 * na);
            memcpy(allele_kind, W.host_ptr(o_ak), na);
        }
        allele_bases_off[na] = (uint32_t)nb;
        if (nb) memcpy(allele_bases, W.host_ptr(o_ab), nb);
        if (maps) {
            const size_t he = rq[4], hb = rq[5];
            memcpy(hap_event_off, W.host_ptr(o_he), 4 * ((size_t)n_haps + 1));
            if (he) {
                memcpy(hap_event_start, W.host_ptr(o_hS), 8 * he);
                memcpy(hap_event_end, W.host_ptr(o_hE), 8 * he);
                memcpy(hap_event_ref_length, W.host_ptr(o_hr), 4 * he);
                memcpy(hap_event_alt_off, W.host_ptr(o_ho), 4 * he);
                memcpy(hap_event_type, W.host_ptr(o_ht), 4 * he);
            }
            hap_event_alt_off[he] = (uint32_t)hb;
            if (hb) memcpy(hap_event_alt, W.host_ptr(o_hb), hb);
        }
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_discover_events", PHMM_FAIL_CODE)
}

}  // extern "C"
