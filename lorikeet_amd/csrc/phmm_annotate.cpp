// phmm_annotate_events (include/phmm.h): host side -- validation, the haplotype -> call allele maps, staging.  The counting
// runs on the device (phmm_annotate_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "phmm_annotate_internal.hpp"
#include "phmm_host.hpp"

using namespace phmm;

namespace {

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct DevGuard {
    int prev = -1, dev;
    explicit DevGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DevGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

bool ok(phmm_handle *h, hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    h->err_code = PHMM_ERR_HIP;
    return false;
}

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
    try {
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
        std::vector<uint64_t> lk_off(n_regions, 0);
        uint64_t n_lk = 0;
        for (uint32_t g = 0; g < n_regions; ++g) {
            if (!region_used[g]) continue;
            lk_off[g] = n_lk;
            n_lk += (uint64_t)(region_read_off[g + 1] - region_read_off[g]) * (region_hap_off[g + 1] - region_hap_off[g]);
        }
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

        DevGuard dg(h->device);
        phmm_handle::AnnWork &W = h->annwork;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the results ------------------------------------------------------------------------------------
        size_t o = 0;
        auto place = [&](size_t bytes) {
            const size_t at = o;
            o += up256(bytes);
            return at;
        };
        const size_t n_es = (size_t)n_events * n_samples, n_bases = with_bq ? read_off[n_reads] : 0;
        const size_t o_rro = place(4ull * (n_regions + 1)), o_rho = place(4ull * (n_regions + 1)), o_lko = place(8ull * n_regions),
                     o_lk = place(8ull * n_lk), o_kp = place(n_reads), o_rs = place(4ull * n_reads), o_st = place(8ull * n_reads),
                     o_en = place(8ull * n_reads), o_mapq = place(n_reads), o_er = place(4ull * n_events), o_emo = place(4ull * n_events),
                     o_map = place(4ull * n_map), o_co = place(4ull * (n_events + 1)), o_es = place(8ull * n_events),
                     o_ee = place(8ull * n_events), o_err = place(8ull * n_events), o_sc = place(sample_called ? n_es : 0),
                     o_nf = place(n_filtered ? 4ull * n_es : 0), o_ro = place(with_bq ? 4ull * (n_reads + 1) : 0), o_bq = place(n_bases),
                     o_cgo = place(with_bq ? 4ull * (n_reads + 1) : 0), o_cg = place(4ull * n_cigar),
                     o_ss = place(with_bq ? 8ull * n_reads : 0), o_ep = place(with_bq ? 8ull * n_events : 0), in_bytes = o;
        const size_t o_af = place(8ull * n_call * n_samples), o_qd = place(8ull * n_events), o_ad = place(4ull * n_call * n_samples),
                     o_dp = place(4ull * n_es), o_ac = place(4ull * n_es), o_idp = place(4ull * n_events), o_qdd = place(4ull * n_events),
                     o_fl = place(4ull * n_events), o_mq = place(n_call), o_obq = place(with_bq ? n_call : 0), total = o;
        if (W.cap < total) {
            (void)hipStreamSynchronize(S);
            if (W.dev) (void)hipFree(W.dev);
            if (W.host) (void)hipHostFree(W.host);
            W.dev = W.host = nullptr;
            W.cap = 0;
            const size_t cap = std::max<size_t>(total + total / 2, 1 << 20);
            if (!ok(h, hipMalloc((void **)&W.dev, cap), "hipMalloc(annotate staging)") ||
                !ok(h, hipHostMalloc((void **)&W.host, cap, hipHostMallocDefault), "hipHostMalloc(annotate staging)"))
                return PHMM_ERR_HIP;
            W.cap = cap;
        }
        auto put = [&](size_t at, const void *src, size_t bytes) {
            if (bytes) memcpy(W.host + at, src, bytes);
        };
        put(o_rro, region_read_off, 4ull * (n_regions + 1));
        put(o_rho, region_hap_off, 4ull * (n_regions + 1));
        put(o_lko, lk_off.data(), 8ull * n_regions);
        for (uint32_t g = 0; g < n_regions; ++g)
            if (region_used[g])
                put(o_lk + 8 * lk_off[g], likelihoods + out_off[g],
                    8ull * (region_read_off[g + 1] - region_read_off[g]) * (region_hap_off[g + 1] - region_hap_off[g]));
        if (keep) put(o_kp, keep, n_reads);
        else if (n_reads) memset(W.host + o_kp, 1, n_reads);
        put(o_rs, read_sample, 4ull * n_reads);
        put(o_st, read_start, 8ull * n_reads);
        put(o_en, read_end, 8ull * n_reads);
        put(o_mapq, mapq, n_reads);
        put(o_er, event_region, 4ull * n_events);
        put(o_emo, map_off.data(), 4ull * n_events);
        put(o_map, hap_call.data(), 4ull * n_map);
        put(o_co, call_off.data(), 4ull * (n_events + 1));
        put(o_es, event_start, 8ull * n_events);
        put(o_ee, event_end, 8ull * n_events);
        put(o_err, log10_p_error, 8ull * n_events);
        if (sample_called) put(o_sc, sample_called, n_es);
        if (n_filtered) put(o_nf, n_filtered, 4ull * n_es);
        if (with_bq) {
            put(o_ro, read_off, 4ull * (n_reads + 1));
            put(o_bq, base_q, n_bases);
            uint32_t *cgo = (uint32_t *)(W.host + o_cgo), at = 0;
            for (uint32_t r = 0; r < n_reads; ++r) {
                cgo[r] = at;
                put(o_cg + 4ull * at, out_cigar + out_cigar_off[r], 4ull * n_out_cigar[r]);
                at += n_out_cigar[r];
            }
            cgo[n_reads] = at;
            put(o_ss, read_soft_start, 8ull * n_reads);
            put(o_ep, event_pos, 8ull * n_events);
        }
        h->stat_staged_bytes += in_bytes;

        AnnotateParams p{};
        p.n_events = n_events;
        p.n_samples = n_samples;
        p.region_read_off = (const uint32_t *)(W.dev + o_rro);
        p.region_hap_off = (const uint32_t *)(W.dev + o_rho);
        p.region_lk_off = (const uint64_t *)(W.dev + o_lko);
        p.likelihoods = (const double *)(W.dev + o_lk);
        p.keep = (const uint8_t *)(W.dev + o_kp);
        p.read_sample = (const uint32_t *)(W.dev + o_rs);
        p.read_start = (const int64_t *)(W.dev + o_st);
        p.read_end = (const int64_t *)(W.dev + o_en);
        p.mapq = (const uint8_t *)(W.dev + o_mapq);
        p.event_region = (const uint32_t *)(W.dev + o_er);
        p.event_map_off = (const uint32_t *)(W.dev + o_emo);
        p.event_hap_call = (const int32_t *)(W.dev + o_map);
        p.call_off = (const uint32_t *)(W.dev + o_co);
        p.event_start = (const int64_t *)(W.dev + o_es);
        p.event_end = (const int64_t *)(W.dev + o_ee);
        p.log10_p_error = (const double *)(W.dev + o_err);
        p.sample_called = sample_called ? (const uint8_t *)(W.dev + o_sc) : nullptr;
        p.n_filtered = n_filtered ? (const uint32_t *)(W.dev + o_nf) : nullptr;
        if (with_bq) {
            p.read_off = (const uint32_t *)(W.dev + o_ro);
            p.base_q = (const uint8_t *)(W.dev + o_bq);
            p.cigar_off = (const uint32_t *)(W.dev + o_cgo);
            p.cigar = (const uint32_t *)(W.dev + o_cg);
            p.read_soft_start = (const int64_t *)(W.dev + o_ss);
            p.event_pos = (const int64_t *)(W.dev + o_ep);
            p.bq = (uint8_t *)(W.dev + o_obq);
        }
        p.af = (double *)(W.dev + o_af);
        p.qd = (double *)(W.dev + o_qd);
        p.ad = (int32_t *)(W.dev + o_ad);
        p.dp = (int32_t *)(W.dev + o_dp);
        p.ac = (uint32_t *)(W.dev + o_ac);
        p.info_dp = (int32_t *)(W.dev + o_idp);
        p.qd_depth = (int32_t *)(W.dev + o_qdd);
        p.flags = (uint32_t *)(W.dev + o_fl);
        p.mq = (uint8_t *)(W.dev + o_mq);
        if (!ok(h, hipMemcpyAsync(W.dev, W.host, in_bytes, hipMemcpyHostToDevice, S), "H2D annotate") ||
            !ok(h, launch_annotate(p, max_call, S), "phmm_annotate_kernel") ||
            !ok(h, hipMemcpyAsync(W.host + o_af, W.dev + o_af, total - o_af, hipMemcpyDeviceToHost, S), "D2H annotate") ||
            !ok(h, hipStreamSynchronize(S), "sync(annotate)"))
            return PHMM_ERR_HIP;
        // per allele and per (sample, allele) results go to the caller's call_allele_off offsets, the rest is dense
        for (uint32_t e = 0; e < n_events; ++e) {
            const size_t C = call_off[e + 1] - call_off[e], at = call_allele_off[e], from = call_off[e];
            if (!C) continue;
            memcpy(ad + at * n_samples, W.host + o_ad + 4 * from * n_samples, 4 * C * n_samples);
            memcpy(af + at * n_samples, W.host + o_af + 8 * from * n_samples, 8 * C * n_samples);
            memcpy(mq + at, W.host + o_mq + from, C);
            if (with_bq) memcpy(bq + at, W.host + o_obq + from, C);
        }
        memcpy(dp, W.host + o_dp, 4 * n_es);
        memcpy(ac, W.host + o_ac, 4 * n_es);
        memcpy(info_dp, W.host + o_idp, 4ull * n_events);
        memcpy(qd_depth, W.host + o_qdd, 4ull * n_events);
        memcpy(qd, W.host + o_qd, 8ull * n_events);
        memcpy(flags, W.host + o_fl, 4ull * n_events);
        return PHMM_OK;
    } catch (const std::bad_alloc &) {
        h->err = "phmm_annotate_events: out of host memory";
        return h->err_code = PHMM_ERR_NO_MEMORY;
    } catch (const std::exception &e) {
        h->err = std::string("phmm_annotate_events: ") + e.what();
        return h->err_code = PHMM_ERR_INTERNAL;
    }
}

}  // extern "C"
