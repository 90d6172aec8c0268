// phmm_trim_regions (include/phmm.h): host side -- validation, the workspace bounds, staging.  Every step runs on the device
// (phmm_events_kernels.hip for the event maps, phmm_trim_kernels.hip); there is no CPU path here.
#include <cstring>
#include <string>
#include <vector>

#include "phmm_host.hpp"
#include "phmm_staging.hpp"
#include "phmm_trim_internal.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_trim_regions: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

// ByteArrayAllele::acceptable_allele_bases (src/model/byte_array_allele.rs:182-207) minus the symbolic and '*' forms
bool accepted(uint8_t b) {
    static const char ok[] = "ACGTNacgtnRYKMSWBDHVU";
    return b && strchr(ok, (int)b);
}

}  // namespace

extern "C" int phmm_trim_regions(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                                 const uint64_t *region_ref_start, const uint64_t *region_active_start,
                                 const uint64_t *region_active_end, const uint64_t *region_padded_start,
                                 const uint64_t *region_padded_end, const uint32_t *region_hap_off, const uint32_t *hap_off,
                                 const uint8_t *hap_bases, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                                 const uint32_t *hap_start_wrt_ref, const uint64_t *hap_loc_start, const uint64_t *hap_loc_end,
                                 const uint8_t *hap_is_ref, uint32_t max_mnp_distance, const uint32_t *padding,
                                 int32_t *region_status, uint8_t *variation_present, uint64_t *variant_start, uint64_t *variant_end,
                                 uint64_t *padded_start, uint64_t *padded_end, uint64_t *new_active_start, uint64_t *new_active_end,
                                 uint64_t *new_padded_start, uint64_t *new_padded_end, int32_t *hap_fate, uint32_t *hap_dup_of,
                                 uint32_t *out_region_hap_off, uint32_t *out_hap_off, uint8_t *out_hap_bases,
                                 uint32_t *out_hap_cigar_off, uint32_t *out_hap_cigar, uint32_t *out_hap_start_wrt_ref,
                                 uint32_t *out_hap_source, uint8_t *out_hap_is_ref, int32_t *out_region_ref_hap) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!padding) return fail(h, "null array (padding)");
        if (!out_region_hap_off || !out_hap_off || !out_hap_cigar_off) return fail(h, "null array (the output offsets)");
        if (!n_regions) {
            out_region_hap_off[0] = out_hap_off[0] = out_hap_cigar_off[0] = 0;
            return PHMM_OK;
        }
        if (!region_ref_off || !region_ref_start || !region_active_start || !region_active_end || !region_padded_start ||
            !region_padded_end || !region_hap_off)
            return fail(h, "null array (region inputs)");
        if (!region_status || !variation_present || !variant_start || !variant_end || !padded_start || !padded_end ||
            !new_active_start || !new_active_end || !new_padded_start || !new_padded_end || !out_region_ref_hap)
            return fail(h, "null array (region outputs)");
        if (region_ref_off[0]) return fail(h, "region_ref_off does not start at 0");
        if (region_hap_off[0]) return fail(h, "region_hap_off does not start at 0");
        for (uint32_t g = 0; g < n_regions; ++g) {
            const auto rg = [g] { return "region " + std::to_string(g) + ": "; };
            if (region_ref_off[g + 1] < region_ref_off[g]) return fail(h, rg() + "region_ref_off not monotonic");
            if (region_hap_off[g + 1] < region_hap_off[g]) return fail(h, rg() + "region_hap_off not monotonic");
            const uint32_t len = region_ref_off[g + 1] - region_ref_off[g], nh = region_hap_off[g + 1] - region_hap_off[g];
            if (len > EV_MAX_REF) return fail(h, rg() + std::to_string(len) + " reference bases, more than " + std::to_string(EV_MAX_REF));
            if (nh > EV_MAX_HAPS) return fail(h, rg() + std::to_string(nh) + " haplotypes, more than " + std::to_string(EV_MAX_HAPS));
            if (region_ref_start[g] >> 62 || region_padded_end[g] >> 62) return fail(h, rg() + "position beyond 2^62");
            // the trimmer's two intersections and its "padded span must include the variant span" hold for every input
            if (!(region_padded_start[g] <= region_active_start[g] && region_active_start[g] <= region_active_end[g] &&
                  region_active_end[g] <= region_padded_end[g]))
                return fail(h, rg() + "the active span is not inside the padded span");
        }
        const uint32_t n_ref = region_ref_off[n_regions], n_haps = region_hap_off[n_regions];
        if (n_ref && !ref_bases) return fail(h, "null array (ref_bases)");
        if (n_haps && (!hap_off || !hap_cigar_off || !hap_start_wrt_ref || !hap_loc_start || !hap_loc_end || !hap_is_ref))
            return fail(h, "null array (haplotype inputs)");
        if (n_haps && (!hap_fate || !hap_dup_of || !out_hap_start_wrt_ref || !out_hap_source || !out_hap_is_ref))
            return fail(h, "null array (haplotype outputs)");
        for (uint32_t i = 0; i < n_ref; ++i)
            if (!accepted(ref_bases[i])) return fail(h, "reference base " + std::to_string(i) + " is not a base the reference's alleles take");
        if (n_haps && hap_off[0]) return fail(h, "hap_off does not start at 0");
        if (n_haps && hap_cigar_off[0]) return fail(h, "hap_cigar_off does not start at 0");
        uint64_t work = 0;
        std::vector<uint32_t> slot(n_haps + 1, 0), hap_region(n_haps);
        for (uint32_t g = 0; g < n_regions; ++g)
            for (uint32_t k = region_hap_off[g]; k < region_hap_off[g + 1]; ++k) hap_region[k] = g;
        for (uint32_t k = 0; k < n_haps; ++k) {
            const auto hp = [k] { return "haplotype " + std::to_string(k) + ": "; };
            if (hap_off[k + 1] < hap_off[k]) return fail(h, hp() + "hap_off not monotonic");
            if (hap_cigar_off[k + 1] < hap_cigar_off[k]) return fail(h, hp() + "hap_cigar_off not monotonic");
            if (hap_loc_end[k] < hap_loc_start[k]) return fail(h, hp() + "its location ends before it starts");
            if (hap_loc_end[k] >> 62) return fail(h, hp() + "position beyond 2^62");
            if ((hap_loc_end[k] - hap_loc_start[k] + hap_start_wrt_ref[k]) >> 32) return fail(h, hp() + "a trimmed start would not fit 32 bits");
            // every event takes a CIGAR element or a haplotype base of its own, every alt byte too (as phmm_discover_events)
            work += (uint64_t)(hap_off[k + 1] - hap_off[k]) + (hap_cigar_off[k + 1] - hap_cigar_off[k]) + 8;
            if (work >> 31) return fail(h, "haplotype bases + CIGAR elements + 8 per haplotype reach 2^31");
            slot[k + 1] = (uint32_t)work;
        }
        const uint32_t n_hap_bases = n_haps ? hap_off[n_haps] : 0, n_cigar = n_haps ? hap_cigar_off[n_haps] : 0;
        if ((n_hap_bases && (!hap_bases || !out_hap_bases)) || (n_cigar && (!hap_cigar || !out_hap_cigar))) return fail(h, "null array (bases, CIGARs)");
        for (uint32_t i = 0; i < n_hap_bases; ++i)
            if (!accepted(hap_bases[i])) return fail(h, "haplotype base " + std::to_string(i) + " is not a base the reference's alleles take");
        for (uint32_t i = 0; i < n_cigar; ++i)
            if ((hap_cigar[i] & 15u) > 8 || !(hap_cigar[i] >> 4))
                return fail(h, "CIGAR element " + std::to_string(i) + ": unknown operator or length 0");

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->trim_staging;
        hipStream_t S = h->streams[0];
        StageLayout L;
        const auto s_ro = L.in(region_ref_off, (size_t)n_regions + 1);
        const auto s_rb = L.in(ref_bases, n_ref);
        const auto s_rs = L.in(region_ref_start, n_regions), s_as = L.in(region_active_start, n_regions), s_ae = L.in(region_active_end, n_regions);
        const auto s_ps = L.in(region_padded_start, n_regions), s_pe = L.in(region_padded_end, n_regions);
        const auto s_rh = L.in(region_hap_off, (size_t)n_regions + 1), s_hr = L.in(hap_region.data(), n_haps);
        const auto s_ho = L.in(hap_off, n_haps ? (size_t)n_haps + 1 : 0);
        const auto s_hb = L.in(hap_bases, n_hap_bases);
        const auto s_co = L.in(hap_cigar_off, n_haps ? (size_t)n_haps + 1 : 0), s_cg = L.in(hap_cigar, n_cigar), s_hs = L.in(hap_start_wrt_ref, n_haps);
        const auto s_ls = L.in(hap_loc_start, n_haps), s_le = L.in(hap_loc_end, n_haps);
        const auto s_ir = L.in(hap_is_ref, n_haps);
        const auto s_sl = L.in(slot.data(), (size_t)n_haps + 1);
        L.end_inputs();
        const auto w_ne = L.scratch<uint32_t>(n_haps), w_na = L.scratch<uint32_t>(n_haps);
        const auto w_hs = L.scratch<int32_t>(n_haps), w_hp = L.scratch<int32_t>(n_haps);
        const auto w_wf = L.scratch<uint32_t>(n_haps), w_wl = L.scratch<uint32_t>(n_haps), w_nc = L.scratch<uint32_t>(n_haps), w_ns = L.scratch<uint32_t>(n_haps);
        const auto w_hl = L.scratch<uint32_t>(n_haps), w_hr2 = L.scratch<uint32_t>(n_haps);
        const auto w_rn = L.scratch<uint32_t>(n_regions);
        const auto w_os = L.scratch<uint32_t>(n_haps), w_ol = L.scratch<uint32_t>(n_haps), w_oc = L.scratch<uint32_t>(n_haps);
        const auto o_st = L.out(region_status, n_regions);
        const auto o_vp = L.out(variation_present, n_regions);
        const auto o_vs = L.out(variant_start, n_regions), o_ve = L.out(variant_end, n_regions), o_ps = L.out(padded_start, n_regions);
        const auto o_pe = L.out(padded_end, n_regions), o_as = L.out(new_active_start, n_regions), o_ae = L.out(new_active_end, n_regions);
        const auto o_qs = L.out(new_padded_start, n_regions), o_qe = L.out(new_padded_end, n_regions);
        const auto o_hf = L.out(hap_fate, n_haps);
        const auto o_hd = L.out(hap_dup_of, n_haps), o_rh = L.out(out_region_hap_off, (size_t)n_regions + 1);
        // the dense arrays are cut by hand below: they are copied as far as they were written
        const auto o_ho = L.out<uint32_t>((size_t)n_haps + 1);
        const auto o_hb = L.out<uint8_t>(n_hap_bases);
        const auto o_co = L.out<uint32_t>((size_t)n_haps + 1), o_cg = L.out<uint32_t>(n_cigar), o_hs = L.out<uint32_t>(n_haps), o_sr = L.out<uint32_t>(n_haps);
        const auto o_ir = L.out<uint8_t>(n_haps);
        const auto o_rr = L.out(out_region_ref_hap, n_regions);
        // The event slots are sized for the worst case and never copied: they lie in the device allocation phmm_discover_events
        // keeps, with the two CIGAR slots of every haplotype behind them.
        StageLayout D;
        const auto w_ev = D.scratch<HapEvent>(work);
        const auto w_al = D.scratch<uint8_t>(work);
        const auto w_ca = D.scratch<uint32_t>(n_cigar), w_cb = D.scratch<uint32_t>(n_cigar);
        if (!h->events_scratch.reserve(h, D, "region trimming workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "region trimming staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;

        EventsParams e{};
        e.n_regions = n_regions;
        e.n_haps = n_haps;
        e.ref_off = W.dev_ptr(s_ro);
        e.ref_bases = W.dev_ptr(s_rb);
        e.region_hap_off = W.dev_ptr(s_rh);
        e.hap_region = W.dev_ptr(s_hr);
        e.hap_off = W.dev_ptr(s_ho);
        e.hap_bases = W.dev_ptr(s_hb);
        e.cigar_off = W.dev_ptr(s_co);
        e.cigar = W.dev_ptr(s_cg);
        e.hap_start = W.dev_ptr(s_hs);
        e.dist = max_mnp_distance;
        e.ws_ev_off = W.dev_ptr(s_sl);
        e.ws_ev = h->events_scratch.ptr(w_ev);
        e.ws_alt = h->events_scratch.ptr(w_al);
        e.hap_n_ev = W.dev_ptr(w_ne);
        e.hap_n_alt = W.dev_ptr(w_na);
        e.hap_status = W.dev_ptr(w_hs);

        TrimParams p{};
        p.n_regions = n_regions;
        p.n_haps = n_haps;
        p.ref_off = e.ref_off;
        p.ref_start = W.dev_ptr(s_rs);
        p.active_start = W.dev_ptr(s_as);
        p.active_end = W.dev_ptr(s_ae);
        p.padded_start = W.dev_ptr(s_ps);
        p.padded_end = W.dev_ptr(s_pe);
        p.region_hap_off = e.region_hap_off;
        p.hap_region = e.hap_region;
        p.hap_off = e.hap_off;
        p.hap_bases = e.hap_bases;
        p.cigar_off = e.cigar_off;
        p.cigar = e.cigar;
        p.hap_start = e.hap_start;
        p.loc_start = W.dev_ptr(s_ls);
        p.loc_end = W.dev_ptr(s_le);
        p.is_ref = W.dev_ptr(s_ir);
        p.pad_snp = padding[0];
        p.pad_indel = padding[1];  // (padding[2], the STR padding, has no input: see include/phmm.h; padding[3] is the legacy trimmer's)
        p.ws_ev_off = e.ws_ev_off;
        p.ws_ev = e.ws_ev;
        p.hap_n_ev = e.hap_n_ev;
        p.hap_status = e.hap_status;
        p.win_first = W.dev_ptr(w_wf);
        p.win_len = W.dev_ptr(w_wl);
        p.new_n_cigar = W.dev_ptr(w_nc);
        p.new_start = W.dev_ptr(w_ns);
        p.hap_panic = W.dev_ptr(w_hp);
        p.ws_cigar_a = h->events_scratch.ptr(w_ca);
        p.ws_cigar_b = h->events_scratch.ptr(w_cb);
        p.hap_below = W.dev_ptr(w_hl);
        p.hap_rep = W.dev_ptr(w_hr2);
        p.region_n_out = W.dev_ptr(w_rn);
        p.out_src = W.dev_ptr(w_os);
        p.out_len = W.dev_ptr(w_ol);
        p.out_n_cigar = W.dev_ptr(w_oc);
        p.region_status = W.dev_ptr(o_st);
        p.variation = W.dev_ptr(o_vp);
        p.variant_start = W.dev_ptr(o_vs);
        p.variant_end = W.dev_ptr(o_ve);
        p.span_start = W.dev_ptr(o_ps);
        p.span_end = W.dev_ptr(o_pe);
        p.new_active_start = W.dev_ptr(o_as);
        p.new_active_end = W.dev_ptr(o_ae);
        p.new_padded_start = W.dev_ptr(o_qs);
        p.new_padded_end = W.dev_ptr(o_qe);
        p.hap_fate = W.dev_ptr(o_hf);
        p.hap_dup_of = W.dev_ptr(o_hd);
        p.out_region_hap_off = W.dev_ptr(o_rh);
        p.out_hap_off = W.dev_ptr(o_ho);
        p.out_bases = W.dev_ptr(o_hb);
        p.out_cigar_off = W.dev_ptr(o_co);
        p.out_cigar = W.dev_ptr(o_cg);
        p.out_start = W.dev_ptr(o_hs);
        p.out_source = W.dev_ptr(o_sr);
        p.out_is_ref = W.dev_ptr(o_ir);
        p.out_region_ref_hap = W.dev_ptr(o_rr);

        if (!stage_round_trip(h, W, L, S, "region trimming", [&] { return hip_ok(h, launch_trim(e, p, S), "phmm_trim kernels"); })) return PHMM_ERR_HIP;
        // the dense arrays: n_out haplotypes, their bases and elements
        const uint32_t n_out = W.host_ptr(o_rh)[n_regions];
        const uint32_t n_out_bases = W.host_ptr(o_ho)[n_out], n_out_cigar = W.host_ptr(o_co)[n_out];
        const auto cut = [&](auto *dst, auto slot, size_t count) {
            if (count) memcpy(dst, W.host_ptr(slot), count * sizeof *dst);
        };
        cut(out_hap_off, o_ho, (size_t)n_out + 1);
        cut(out_hap_bases, o_hb, n_out_bases);
        cut(out_hap_cigar_off, o_co, (size_t)n_out + 1);
        cut(out_hap_cigar, o_cg, n_out_cigar);
        cut(out_hap_start_wrt_ref, o_hs, n_out);
        cut(out_hap_source, o_sr, n_out);
        cut(out_hap_is_ref, o_ir, n_out);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_trim_regions", PHMM_FAIL_CODE)
}
