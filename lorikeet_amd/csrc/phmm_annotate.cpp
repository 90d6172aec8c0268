// phmm_annotate_events (include/phmm.h): host side -- validation, the haplotype -> call allele maps, staging.  The counting
// runs on the device (phmm_annotate_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "phmm_annotate_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_annotate_events: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" {

int phmm_annotate_events(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                         const uint64_t *out_off, const double *likelihoods, const uint8_t *keep, const uint32_t *read_sample,
                         const int64_t *read_start, const int64_t *read_end, const uint8_t *mapq, uint32_t n_samples,
                         uint32_t n_events, const uint32_t *event_region, const uint32_t *event_allele_off,
                         const int64_t *event_start, const int64_t *event_end, const int32_t *event_hap_allele,
                         const uint32_t *call_allele_off, const uint32_t *call_allele, const uint32_t *read_off,
                         const uint8_t *base_q, const uint64_t *out_cigar_off, const uint32_t *out_cigar,
                         const uint32_t *n_out_cigar, const int64_t *read_soft_start, const int64_t *event_pos,
                         const uint8_t *sample_called, const double *log10_p_error, const uint32_t *n_filtered, int32_t *ad,
                         int32_t *dp, double *af, uint32_t *ac, uint8_t *mq, uint8_t *bq, int32_t *info_dp, int32_t *qd_depth,
                         double *qd, uint32_t *flags) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        if (!n_events) return PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!region_read_off || !region_hap_off || !out_off || !likelihoods || !event_region || !event_allele_off || !event_start ||
            !event_end || !event_hap_allele || !call_allele_off || !log10_p_error || !ad || !dp || !af || !ac || !mq || !info_dp ||
            !qd_depth || !qd || !flags)
            return fail(h, "null array");
        const int n_bq = !!read_off + !!base_q + !!out_cigar_off + !!out_cigar + !!n_out_cigar + !!read_soft_start + !!event_pos + !!bq;
        if (n_bq != 0 && n_bq != 8)
            return fail(h, "the BQ arrays (read_off, base_q, out_cigar_off, out_cigar, n_out_cigar, read_soft_start, event_pos, bq) "
                           "must be given together or not at all");
        const bool with_bq = n_bq == 8;
        if (region_read_off[0] != 0 || region_hap_off[0] != 0) return fail(h, "region offset arrays must start at 0");
        for (uint32_t g = 0; g < n_regions; ++g)
            if (region_read_off[g + 1] < region_read_off[g] || region_hap_off[g + 1] < region_hap_off[g])
                return fail(h, "region offsets not monotonic at region " + std::to_string(g));
        const uint32_t n_reads = n_regions ? region_read_off[n_regions] : 0;
        if (n_reads && (!read_sample || !read_start || !read_end || !mapq)) return fail(h, "null array");
        for (uint32_t r = 0; r < n_reads; ++r)
            if (read_sample[r] >= n_samples) return fail(h, "read " + std::to_string(r) + ": read_sample outside [0, n_samples)");
        uint64_t n_cigar = 0;
        if (with_bq) {
            if (read_off[0] != 0) return fail(h, "read_off must start at 0");
            for (uint32_t r = 0; r < n_reads; ++r) {
                if (read_off[r + 1] < read_off[r]) return fail(h, "read " + std::to_string(r) + ": read_off not monotonic");
                if (out_cigar_off[r + 1] < out_cigar_off[r] || n_out_cigar[r] > out_cigar_off[r + 1] - out_cigar_off[r])
                    return fail(h, "read " + std::to_string(r) + ": n_out_cigar beyond its out_cigar_off slot");
                n_cigar += n_out_cigar[r];
            }
            if (n_cigar > UINT32_MAX) return fail(h, "CIGARs beyond 2^32 elements");
        }
        std::vector<uint32_t> map_off(n_events), call_off(n_events + 1, 0);
        std::vector<char> region_used(n_regions, 0);
        uint64_t n_map = 0;
        uint32_t max_call = 0;
        if (!call_allele) {  // (allowed when every event's list is empty)
            for (uint32_t e = 0; e < n_events; ++e)
                if (call_allele_off[e + 1] != call_allele_off[e]) return fail(h, "null array");
        }
        for (uint32_t e = 0; e < n_events; ++e) {
            const std::string ev = "event " + std::to_string(e) + ": ";
            if (event_region[e] >= n_regions) return fail(h, ev + "event_region outside [0, n_regions)");
            if (event_allele_off[e + 1] < event_allele_off[e]) return fail(h, ev + "event_allele_off not monotonic");
            const uint32_t A = event_allele_off[e + 1] - event_allele_off[e];
            if (!A) return fail(h, ev + "no alleles");
            if (A > ANN_MAX_ALLELES) return fail(h, ev + std::to_string(A) + " alleles, more than " + std::to_string(ANN_MAX_ALLELES));
            const uint32_t g = event_region[e], nh = region_hap_off[g + 1] - region_hap_off[g];
            for (uint32_t k = 0; k < nh; ++k) {
                const int32_t a = event_hap_allele[n_map + k];
                if (a < -1 || a >= (int32_t)A) return fail(h, ev + "haplotype " + std::to_string(k) + " maps outside [-1, A_e)");
            }
            if (call_allele_off[e + 1] < call_allele_off[e]) return fail(h, ev + "call_allele_off not monotonic");
            const uint32_t C = call_allele_off[e + 1] - call_allele_off[e];
            const uint32_t *ca = call_allele + call_allele_off[e];
            if (C && ca[0] != 0) return fail(h, ev + "call_allele[0] is not 0 (the reference)");
            for (uint32_t c = 0; c < C; ++c) {
                if (ca[c] >= A) return fail(h, ev + "call allele " + std::to_string(c) + " outside [0, A_e)");
                if (c && ca[c] <= ca[c - 1]) return fail(h, ev + "call alleles not strictly increasing");
            }
            if (n_map > UINT32_MAX) return fail(h, "haplotype -> allele maps beyond 2^32 entries");
            map_off[e] = (uint32_t)n_map;
            n_map += nh;
            if ((uint64_t)call_off[e] + C > UINT32_MAX) return fail(h, "call alleles beyond 2^32 entries");
            call_off[e + 1] = call_off[e] + C;
            if (C) region_used[g] = 1;
            max_call = std::max(max_call, C);
        }
        const size_t n_call = call_off[n_events];
        const LikelihoodGather lks(n_regions, region_read_off, region_hap_off, region_used);
        // the subset map of the call (haplotype_caller_genotyping_engine.rs:376-384) composed with the event's: haplotype -> index in
        // the call, -1 for a haplotype on no allele or on one the call leaves out
        std::vector<int32_t> hap_call(n_map), inverse(ANN_MAX_ALLELES);
        for (uint32_t e = 0; e < n_events; ++e) {
            const uint32_t A = event_allele_off[e + 1] - event_allele_off[e], C = call_off[e + 1] - call_off[e];
            const uint32_t g = event_region[e], nh = region_hap_off[g + 1] - region_hap_off[g];
            std::fill(inverse.begin(), inverse.begin() + A, -1);
            for (uint32_t c = 0; c < C; ++c) inverse[call_allele[call_allele_off[e] + c]] = (int32_t)c;
            for (uint32_t k = 0; k < nh; ++k) {
                const int32_t a = event_hap_allele[map_off[e] + k];
                hap_call[map_off[e] + k] = a < 0 ? -1 : inverse[a];
            }
        }

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->annotate_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the results ------------------------------------------------------------------------------------
        const size_t n_es = (size_t)n_events * n_samples, n_bases = with_bq ? read_off[n_reads] : 0;
        StageLayout L;
        const auto s_rro = L.in(region_read_off, n_regions + 1), s_rho = L.in(region_hap_off, n_regions + 1);
        const auto s_lko = L.in(lks.off.data(), n_regions);
        const auto s_lk = L.in<double>(lks.n);
        const auto s_kp = L.in<uint8_t>(n_reads);
        const auto s_rs = L.in(read_sample, n_reads);
        const auto s_st = L.in(read_start, n_reads), s_en = L.in(read_end, n_reads);
        const auto s_mapq = L.in(mapq, n_reads);
        const auto s_er = L.in(event_region, n_events), s_emo = L.in(map_off.data(), n_events);
        const auto s_map = L.in(hap_call.data(), n_map);
        const auto s_co = L.in(call_off.data(), n_events + 1);
        const auto s_es = L.in(event_start, n_events), s_ee = L.in(event_end, n_events);
        const auto s_err = L.in(log10_p_error, n_events);
        const auto s_sc = L.in(sample_called, sample_called ? n_es : 0);
        const auto s_nf = L.in(n_filtered, n_filtered ? n_es : 0);
        const auto s_ro = L.in(read_off, with_bq ? n_reads + 1 : 0);
        const auto s_bq = L.in(base_q, n_bases);
        const auto s_cgo = L.in<uint32_t>(with_bq ? n_reads + 1 : 0), s_cg = L.in<uint32_t>(n_cigar);  // the CIGARs, repacked densely below
        const auto s_ss = L.in(read_soft_start, with_bq ? n_reads : 0), s_ep = L.in(event_pos, with_bq ? n_events : 0);
        L.end_inputs();
        const auto s_af = L.out<double>(n_call * n_samples), s_qd = L.out<double>(n_events);
        const auto s_ad = L.out<int32_t>(n_call * n_samples), s_dp = L.out<int32_t>(n_es);
        const auto s_ac = L.out<uint32_t>(n_es);
        const auto s_idp = L.out<int32_t>(n_events), s_qdd = L.out<int32_t>(n_events);
        const auto s_fl = L.out<uint32_t>(n_events);
        const auto s_mq = L.out<uint8_t>(n_call), s_obq = L.out<uint8_t>(with_bq ? n_call : 0);
        if (!W.reserve(h, L, "annotate staging")) return PHMM_ERR_HIP;
        lks.into(W.host_ptr(s_lk), W.host_ptr(s_kp), out_off, likelihoods, keep);
        if (with_bq) {
            uint32_t *cgo = W.host_ptr(s_cgo), *cg = W.host_ptr(s_cg), at = 0;
            for (uint32_t r = 0; r < n_reads; ++r) {
                cgo[r] = at;
                if (n_out_cigar[r]) memcpy(cg + at, out_cigar + out_cigar_off[r], 4ull * n_out_cigar[r]);
                at += n_out_cigar[r];
            }
            cgo[n_reads] = at;
        }
        h->stat_staged_bytes += L.in_bytes;

        AnnotateParams p{};
        p.n_events = n_events;
        p.n_samples = n_samples;
        p.region_read_off = W.dev_ptr(s_rro);
        p.region_hap_off = W.dev_ptr(s_rho);
        p.region_lk_off = W.dev_ptr(s_lko);
        p.likelihoods = W.dev_ptr(s_lk);
        p.keep = W.dev_ptr(s_kp);
        p.read_sample = W.dev_ptr(s_rs);
        p.read_start = W.dev_ptr(s_st);
        p.read_end = W.dev_ptr(s_en);
        p.mapq = W.dev_ptr(s_mapq);
        p.event_region = W.dev_ptr(s_er);
        p.event_map_off = W.dev_ptr(s_emo);
        p.event_hap_call = W.dev_ptr(s_map);
        p.call_off = W.dev_ptr(s_co);
        p.event_start = W.dev_ptr(s_es);
        p.event_end = W.dev_ptr(s_ee);
        p.log10_p_error = W.dev_ptr(s_err);
        p.sample_called = sample_called ? W.dev_ptr(s_sc) : nullptr;
        p.n_filtered = n_filtered ? W.dev_ptr(s_nf) : nullptr;
        if (with_bq) {
            p.read_off = W.dev_ptr(s_ro);
            p.base_q = W.dev_ptr(s_bq);
            p.cigar_off = W.dev_ptr(s_cgo);
            p.cigar = W.dev_ptr(s_cg);
            p.read_soft_start = W.dev_ptr(s_ss);
            p.event_pos = W.dev_ptr(s_ep);
            p.bq = W.dev_ptr(s_obq);
        }
        p.af = W.dev_ptr(s_af);
        p.qd = W.dev_ptr(s_qd);
        p.ad = W.dev_ptr(s_ad);
        p.dp = W.dev_ptr(s_dp);
        p.ac = W.dev_ptr(s_ac);
        p.info_dp = W.dev_ptr(s_idp);
        p.qd_depth = W.dev_ptr(s_qdd);
        p.flags = W.dev_ptr(s_fl);
        p.mq = W.dev_ptr(s_mq);
        if (!stage_round_trip(h, W, L, S, "annotate", [&] { return hip_ok(h, launch_annotate(p, max_call, S), "phmm_annotate_kernel"); })) return PHMM_ERR_HIP;
        // per allele and per (sample, allele) results go to the caller's call_allele_off offsets, the rest is dense
        for (uint32_t e = 0; e < n_events; ++e) {
            const size_t C = call_off[e + 1] - call_off[e], at = call_allele_off[e], from = call_off[e];
            if (!C) continue;
            memcpy(ad + at * n_samples, W.host_ptr(s_ad) + from * n_samples, 4 * C * n_samples);
            memcpy(af + at * n_samples, W.host_ptr(s_af) + from * n_samples, 8 * C * n_samples);
            memcpy(mq + at, W.host_ptr(s_mq) + from, C);
            if (with_bq) memcpy(bq + at, W.host_ptr(s_obq) + from, C);
        }
        memcpy(dp, W.host_ptr(s_dp), 4 * n_es);
        memcpy(ac, W.host_ptr(s_ac), 4 * n_es);
        memcpy(info_dp, W.host_ptr(s_idp), 4ull * n_events);
        memcpy(qd_depth, W.host_ptr(s_qdd), 4ull * n_events);
        memcpy(qd, W.host_ptr(s_qd), 8ull * n_events);
        memcpy(flags, W.host_ptr(s_fl), 4ull * n_events);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_annotate_events", PHMM_FAIL_CODE)
}

}  // extern "C"
