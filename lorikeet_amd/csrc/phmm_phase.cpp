// phmm_phase_calls (include/phmm.h): host side -- validation and staging.  Every step runs on the device
// (phmm_phase_kernels.hip); there is no CPU path here.
#include <cstring>
#include <string>
#include <vector>

#include "phmm_host.hpp"
#include "phmm_phase_internal.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_phase_calls: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int phmm_phase_calls(phmm_handle *h, uint32_t n_regions, const uint32_t *region_event_off, const uint32_t *region_hap_off,
                                const uint32_t *event_allele_off, const int32_t *event_hap_allele, const int64_t *vc_start,
                                const uint32_t *allele_length, const uint8_t *allele_kind, const uint32_t *allele_bases_off,
                                const uint8_t *allele_bases, const uint32_t *hap_event_off, const int64_t *hap_event_start,
                                const uint32_t *hap_event_alt_off, const uint8_t *hap_event_alt, const uint32_t *call_allele_off,
                                const uint32_t *call_allele, uint32_t n_samples, uint32_t ploidy, const int32_t *gt, uint32_t flags,
                                uint32_t *call_rev_trim, int64_t *call_end, uint32_t *phase_n_haps, uint8_t *hap_in_call,
                                int32_t *phase_group, uint8_t *phase_gt, int32_t *phase_leader, int64_t *phase_set,
                                uint32_t *region_alt_haps, uint32_t *region_phase_flags, uint8_t *is_phased, int32_t *gt_phased) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (flags & ~(uint32_t)PHMM_PH_NO_TRIM) return fail(h, "flags holds bits outside PHMM_PH_NO_TRIM");
        if (gt && (!is_phased || !gt_phased)) return fail(h, "a required pointer is NULL (gt without is_phased or gt_phased)");
        if (!gt && (is_phased || gt_phased)) return fail(h, "is_phased or gt_phased without gt");
        if (gt && !ploidy) return fail(h, "ploidy is 0 with gt given");
        if (!n_regions) return PHMM_OK;
        if (!region_event_off || !region_hap_off || !region_alt_haps || !region_phase_flags)
            return fail(h, "a required pointer is NULL (region arrays)");
        if (region_event_off[0]) return fail(h, "region_event_off does not start at 0");
        if (region_hap_off[0]) return fail(h, "region_hap_off does not start at 0");
        uint64_t n_map = 0;
        for (uint32_t g = 0; g < n_regions; ++g) {
            const auto rg = [g] { return "region " + std::to_string(g) + ": "; };   // (made only for a failure)
            if (region_event_off[g + 1] < region_event_off[g]) return fail(h, rg() + "region_event_off decreases");
            if (region_hap_off[g + 1] < region_hap_off[g]) return fail(h, rg() + "region_hap_off decreases");
            const uint32_t nh = region_hap_off[g + 1] - region_hap_off[g];
            if (nh > PH_MAX_HAPS) return fail(h, rg() + std::to_string(nh) + " haplotypes, more than " + std::to_string(PH_MAX_HAPS));
            n_map += (uint64_t)nh * (region_event_off[g + 1] - region_event_off[g]);
        }
        if (n_map >> 32) return fail(h, "event_hap_allele would hold 2^32 entries or more");
        const uint32_t n_events = region_event_off[n_regions], n_haps = region_hap_off[n_regions];
        uint32_t n_alleles = 0, n_call = 0, n_allele_bytes = 0, n_hap_events = 0, n_hap_bytes = 0;
        std::vector<uint32_t> event_region(n_events), event_map_off(n_events);
        if (n_events) {
            if (!event_allele_off || !vc_start || !allele_length || !allele_kind || !allele_bases_off || !call_allele_off ||
                !call_rev_trim || !call_end || !phase_n_haps || !phase_group || !phase_gt || !phase_leader || !phase_set)
                return fail(h, "a required pointer is NULL (event arrays)");
            if (n_map && !event_hap_allele) return fail(h, "a required pointer is NULL (event_hap_allele)");
            if (event_allele_off[0]) return fail(h, "event_allele_off does not start at 0");
            if (call_allele_off[0]) return fail(h, "call_allele_off does not start at 0");
            if (allele_bases_off[0]) return fail(h, "allele_bases_off does not start at 0");
            for (uint32_t e = 0; e < n_events; ++e) {
                const auto ev = [e] { return "event " + std::to_string(e) + ": "; };
                if (event_allele_off[e + 1] < event_allele_off[e]) return fail(h, ev() + "event_allele_off decreases");
                if (call_allele_off[e + 1] < call_allele_off[e]) return fail(h, ev() + "call_allele_off decreases");
            }
            n_alleles = event_allele_off[n_events];
            n_call = call_allele_off[n_events];
            if (n_call && !call_allele) return fail(h, "a required pointer is NULL (call_allele)");
            for (uint32_t a = 0; a < n_alleles; ++a) {
                if (allele_bases_off[a + 1] < allele_bases_off[a]) return fail(h, "allele " + std::to_string(a) + ": allele_bases_off decreases");
                if (allele_kind[a] > PH_KIND_NON_REF) return fail(h, "allele " + std::to_string(a) + ": unknown kind " + std::to_string(allele_kind[a]));
            }
            n_allele_bytes = allele_bases_off[n_alleles];
            if (n_allele_bytes && !allele_bases) return fail(h, "a required pointer is NULL (allele_bases)");
            uint32_t m = 0;
            for (uint32_t g = 0; g < n_regions; ++g)
                for (uint32_t e = region_event_off[g]; e < region_event_off[g + 1]; ++e) {
                    event_region[e] = g;
                    event_map_off[e] = m;
                    m += region_hap_off[g + 1] - region_hap_off[g];
                }
            for (uint32_t e = 0; e < n_events; ++e) {
                const auto ev = [e] { return "event " + std::to_string(e) + ": "; };
                const uint32_t a0 = event_allele_off[e], A = event_allele_off[e + 1] - a0;
                const uint32_t c0 = call_allele_off[e], C = call_allele_off[e + 1] - c0;
                if (!C) continue;
                if (call_allele[c0]) return fail(h, ev() + "the call does not start with allele 0");
                for (uint32_t k = 0; k < C; ++k) {
                    const auto ca = [&] { return ev() + "call allele " + std::to_string(k) + " "; };
                    const uint32_t c = call_allele[c0 + k];
                    if (k && c <= call_allele[c0 + k - 1]) return fail(h, ca() + "is not above the one before it");
                    if (c >= A) return fail(h, ca() + "reaches A_e (" + std::to_string(A) + ")");
                    if (allele_kind[a0 + c] == PH_KIND_NON_REF) continue;   // symbolic: no base of it is read
                    if (!allele_length[a0 + c]) return fail(h, ca() + "has length 0");
                    if (allele_length[a0 + c] > allele_bases_off[a0 + c + 1] - allele_bases_off[a0 + c]) return fail(h, ca() + "is longer than its bytes");
                }
                if (allele_kind[a0] != PH_KIND_PLAIN) return fail(h, ev() + "the reference allele is not plain");
                if (gt)
                    for (uint32_t s = 0; s < n_samples; ++s)
                        for (uint32_t k = 0; k < ploidy; ++k) {
                            const int32_t v = gt[((uint64_t)e * n_samples + s) * ploidy + k];
                            if (v < -1 || v >= (int64_t)C)
                                return fail(h, ev() + "sample " + std::to_string(s) + ": gt entry " + std::to_string(v) + " is outside [-1, " + std::to_string(C) + ")");
                        }
            }
            if (n_haps) {
                if (!hap_event_off) return fail(h, "a required pointer is NULL (hap_event_off)");
                if (hap_event_off[0]) return fail(h, "hap_event_off does not start at 0");
                for (uint32_t k = 0; k < n_haps; ++k)
                    if (hap_event_off[k + 1] < hap_event_off[k]) return fail(h, "haplotype " + std::to_string(k) + ": hap_event_off decreases");
                n_hap_events = hap_event_off[n_haps];
                if (n_hap_events) {
                    if (!hap_event_start || !hap_event_alt_off) return fail(h, "a required pointer is NULL (hap_event_start, hap_event_alt_off)");
                    if (hap_event_alt_off[0]) return fail(h, "hap_event_alt_off does not start at 0");
                    for (uint32_t i = 0; i < n_hap_events; ++i)
                        if (hap_event_alt_off[i + 1] < hap_event_alt_off[i]) return fail(h, "haplotype event " + std::to_string(i) + ": hap_event_alt_off decreases");
                    n_hap_bytes = hap_event_alt_off[n_hap_events];
                    if (n_hap_bytes && !hap_event_alt) return fail(h, "a required pointer is NULL (hap_event_alt)");
                    for (uint32_t k = 0; k < n_haps; ++k)
                        for (uint32_t i = hap_event_off[k] + 1; i < hap_event_off[k + 1]; ++i)
                            if (hap_event_start[i] <= hap_event_start[i - 1])
                                return fail(h, "haplotype " + std::to_string(k) + ": its events do not ascend by start (event " + std::to_string(i - hap_event_off[k]) + ")");
                }
            }
        }
        const uint64_t n_gt = gt ? (uint64_t)n_events * n_samples : 0;

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->phase_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs; the bitsets lie in the device-only workspace ----------------------------------
        StageLayout L;
        const auto s_re = L.in(region_event_off, (size_t)n_regions + 1), s_rh = L.in(region_hap_off, (size_t)n_regions + 1);
        const auto s_er = L.in(event_region.data(), n_events), s_em = L.in(event_map_off.data(), n_events);
        const auto s_ea = L.in(event_allele_off, n_events ? (size_t)n_events + 1 : 0);
        const auto s_hm = L.in(event_hap_allele, n_events ? n_map : 0);
        const auto s_vs = L.in(vc_start, n_events);
        const auto s_al = L.in(allele_length, n_alleles);
        const auto s_ak = L.in(allele_kind, n_alleles);
        const auto s_ao = L.in(allele_bases_off, n_events ? (size_t)n_alleles + 1 : 0);
        const auto s_ab = L.in(allele_bases, n_allele_bytes);
        const bool maps = n_events && n_haps;
        const auto s_he = L.in(hap_event_off, maps ? (size_t)n_haps + 1 : 0);
        const auto s_hs = L.in(hap_event_start, n_hap_events);
        const auto s_ho = L.in(hap_event_alt_off, n_hap_events ? (size_t)n_hap_events + 1 : 0);
        const auto s_hb = L.in(hap_event_alt, n_hap_bytes);
        const auto s_co = L.in(call_allele_off, n_events ? (size_t)n_events + 1 : 0), s_ca = L.in(call_allele, n_call);
        const auto s_gt = L.in(gt, n_gt * ploidy);
        L.end_inputs();
        const auto o_rt = L.out(call_rev_trim, n_events);
        const auto o_ce = L.out(call_end, n_events);
        const auto o_nh = L.out(phase_n_haps, n_events);
        const auto o_hc = L.out(hap_in_call, hap_in_call && n_events ? n_map : 0);  // (not given: no slot, and the kernels see null)
        const auto o_pg = L.out(phase_group, n_events);
        const auto o_pt = L.out(phase_gt, n_events);
        const auto o_pl = L.out(phase_leader, n_events);
        const auto o_ps = L.out(phase_set, n_events);
        const auto o_ah = L.out(region_alt_haps, n_regions), o_pf = L.out(region_phase_flags, n_regions);
        const auto o_ip = L.out(is_phased, n_gt);
        const auto o_gp = L.out(gt_phased, n_gt * ploidy);
        StageLayout D;  // the device-only workspace
        const auto w_rc = D.scratch<unsigned long long>((size_t)n_regions * PH_WORDS);
        const auto w_st = D.scratch<unsigned long long>((size_t)n_events * PH_WORDS);
        const auto w_gl = D.scratch<uint32_t>(n_events);
        if (!h->phase_scratch.reserve(h, D, "phasing workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "phasing staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->phase_scratch;

        PhaseParams p{};
        p.n_regions = n_regions;
        p.n_events = n_events;
        p.n_samples = n_samples;
        p.ploidy = ploidy;
        p.flags = flags;
        p.region_event_off = W.dev_ptr(s_re);
        p.region_hap_off = W.dev_ptr(s_rh);
        p.event_region = W.dev_ptr(s_er);
        p.event_map_off = W.dev_ptr(s_em);
        p.event_allele_off = W.dev_ptr(s_ea);
        p.event_hap_allele = W.dev_ptr(s_hm);
        p.vc_start = W.dev_ptr(s_vs);
        p.allele_length = W.dev_ptr(s_al);
        p.allele_kind = W.dev_ptr(s_ak);
        p.allele_bases_off = W.dev_ptr(s_ao);
        p.allele_bases = W.dev_ptr(s_ab);
        p.hap_event_off = W.dev_ptr(s_he);
        p.hap_event_start = W.dev_ptr(s_hs);
        p.hap_event_alt_off = W.dev_ptr(s_ho);
        p.hap_event_alt = W.dev_ptr(s_hb);
        p.call_allele_off = W.dev_ptr(s_co);
        p.call_allele = W.dev_ptr(s_ca);
        p.gt = gt ? W.dev_ptr(s_gt) : nullptr;
        p.region_called = ws.ptr(w_rc);
        p.sets = ws.ptr(w_st);
        p.group_leader = ws.ptr(w_gl);
        p.call_rev_trim = W.dev_ptr_or_null(o_rt);
        p.call_end = W.dev_ptr_or_null(o_ce);
        p.phase_n_haps = W.dev_ptr_or_null(o_nh);
        p.hap_in_call = W.dev_ptr_or_null(o_hc);
        p.phase_group = W.dev_ptr_or_null(o_pg);
        p.phase_gt = W.dev_ptr_or_null(o_pt);
        p.phase_leader = W.dev_ptr_or_null(o_pl);
        p.phase_set = W.dev_ptr_or_null(o_ps);
        p.region_alt_haps = W.dev_ptr_or_null(o_ah);
        p.region_phase_flags = W.dev_ptr_or_null(o_pf);
        p.is_phased = W.dev_ptr_or_null(o_ip);
        p.gt_phased = W.dev_ptr_or_null(o_gp);
        // gt with no sample or no event has nothing to write: the stage is skipped as without gt
        if (!n_gt) p.gt = nullptr;

        if (!stage_round_trip(h, W, L, S, "phasing", [&] { return hip_ok(h, launch_phase(p, S), "phasing kernels"); })) return PHMM_ERR_HIP;
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_phase_calls", PHMM_FAIL_CODE)
}
