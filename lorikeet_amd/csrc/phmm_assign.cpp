// phmm_assign_genotypes (include/phmm.h): host side -- validation, the allele types and prior tables, the genotype tables,
// staging.  The arithmetic runs on the device (phmm_assign_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "phmm_assign_internal.hpp"
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
    h->err = "phmm_assign_genotypes: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" {

int phmm_assign_genotypes(phmm_handle *h, uint32_t n_events, uint32_t n_samples, uint32_t ploidy, const uint32_t *event_allele_off,
                          const uint32_t *allele_length, const uint8_t *allele_kind, const uint64_t *pl_off, const int32_t *pl,
                          const uint32_t *call_allele_off, const uint32_t *call_allele, uint32_t method, double log10_snp_het,
                          double log10_indel_het, const uint8_t *site_monomorphic, const uint64_t *sub_pl_off, int32_t *sub_pl,
                          int32_t *gt, int32_t *gq, double *log10_gq, uint8_t *sample_called, uint8_t *sample_flags, double *gp,
                          double *pg, double *log10_p_error_posterior) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    try {
        h->err_code = PHMM_OK;
        if (!n_events) return PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (method != PHMM_GT_USE_PLS && method != PHMM_GT_USE_POSTERIORS) return fail(h, "unknown method " + std::to_string(method));
        const bool posteriors = method == PHMM_GT_USE_POSTERIORS;
        if (!event_allele_off || !pl_off || !call_allele_off || !sub_pl_off || !gt || !gq || !sample_called || !sample_flags)
            return fail(h, "null array");
        if (posteriors && (!allele_length || !gp || !pg || !log10_p_error_posterior))
            return fail(h, "null array (the posterior method needs allele_length, gp, pg and log10_p_error_posterior)");
        if (!ploidy) return fail(h, "ploidy must be at least 1");
        if (!call_allele) {  // (allowed when every event's list is empty)
            for (uint32_t e = 0; e < n_events; ++e)
                if (call_allele_off[e + 1] != call_allele_off[e]) return fail(h, "null array");
        }
        std::vector<uint32_t> computed, G(n_events, 0), Gn(n_events, 0);
        uint32_t max_alleles = 0, max_call = 0;
        for (uint32_t e = 0; e < n_events; ++e) {
            const std::string ev = "event " + std::to_string(e) + ": ";
            if (event_allele_off[e + 1] < event_allele_off[e]) return fail(h, ev + "event_allele_off not monotonic");
            if (pl_off[e + 1] < pl_off[e]) return fail(h, ev + "pl_off not monotonic");
            if (call_allele_off[e + 1] < call_allele_off[e]) return fail(h, ev + "call_allele_off not monotonic");
            if (sub_pl_off[e + 1] < sub_pl_off[e]) return fail(h, ev + "sub_pl_off not monotonic");
            const uint32_t a0 = event_allele_off[e], A = event_allele_off[e + 1] - a0;
            if (A < 2) return fail(h, ev + "fewer than 2 alleles");
            const uint32_t C = call_allele_off[e + 1] - call_allele_off[e];
            if (!C) continue;  // not called: nothing of the event is read
            const uint32_t *ca = call_allele + call_allele_off[e];
            if (ca[0] != 0) return fail(h, ev + "call_allele[0] is not 0 (the reference)");
            for (uint32_t c = 0; c < C; ++c) {
                if (ca[c] >= A) return fail(h, ev + "call allele " + std::to_string(c) + " outside [0, A_e)");
                if (c && ca[c] <= ca[c - 1]) return fail(h, ev + "call alleles not strictly increasing");
                if (allele_kind && allele_kind[a0 + ca[c]] > PHMM_AF_KIND_NON_REF)
                    return fail(h, ev + "allele " + std::to_string(ca[c]) + ": unknown kind");
                // calculate_allele_types (genotype_prior_calculator.rs:201-228) panics on a called symbolic allele
                if (posteriors && allele_kind && allele_kind[a0 + ca[c]] == PHMM_AF_KIND_NON_REF)
                    return fail(h, ev + "the posterior method cannot take <NON_REF> in the call");
            }
            G[e] = phmm_genotype_count(ploidy, A);
            if (G[e] > AS_MAX_GENOTYPES)
                return fail(h, ev + std::to_string(G[e]) + " genotypes, more than " + std::to_string(AS_MAX_GENOTYPES));
            if (pl_off[e + 1] - pl_off[e] < (uint64_t)n_samples * G[e]) return fail(h, ev + "pl_off slot smaller than n_samples x genotypes");
            if (C < 2) continue;  // subset_to_ref_only: no PLs
            Gn[e] = phmm_genotype_count(ploidy, C);
            if (sub_pl_off[e + 1] - sub_pl_off[e] < (uint64_t)n_samples * Gn[e])
                return fail(h, ev + "sub_pl_off slot smaller than n_samples x genotypes of the call");
            if (n_samples) {
                computed.push_back(e);
                max_alleles = std::max(max_alleles, A);
                max_call = std::max(max_call, C);
            }
        }
        const uint32_t n_c = (uint32_t)computed.size();
        if (n_c && (!pl || !sub_pl)) return fail(h, "null array");

        // ---- events that are not computed: not called, or the reference alone (subset_to_ref_only, variant_context.rs:586-619) ----
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (uint32_t e = 0; e < n_events; ++e) {
            const uint32_t C = call_allele_off[e + 1] - call_allele_off[e];
            if (posteriors && (C < 2 || !n_samples)) log10_p_error_posterior[e] = C ? nan : 0.0;
            if (C >= 2) continue;
            const size_t es = (size_t)e * n_samples;
            std::fill(gt + es * ploidy, gt + (es + n_samples) * ploidy, 0);
            for (size_t s = es; s < es + n_samples; ++s) {
                gq[s] = C ? -1 : 0;
                if (log10_gq) log10_gq[s] = C ? nan : 0.0;
                sample_called[s] = C ? 1 : 0;
                sample_flags[s] = C ? PHMM_GT_SAMPLE_REF_ONLY : 0;
            }
        }
        if (!n_c) return PHMM_OK;

        // ---- the tables: compositions over the largest call, the offset table over the most alleles ------------------------
        const auto &T = genotype_table_of(h, ploidy, max_call);
        const uint32_t stride = max_alleles + 1;
        const auto off = genotype_offset_table(ploidy, max_alleles);
        std::vector<uint32_t> rank((size_t)(ploidy + 1) * stride);  // row p at p * stride
        for (uint32_t p = 0; p <= ploidy; ++p)
            for (uint32_t a = 0; a <= max_alleles; ++a) rank[(size_t)p * stride + a] = (uint32_t)off[p][a];

        // ---- the computed events, densely ------------------------------------------------------------------------------------
        std::vector<uint32_t> c_call_off(n_c + 1, 0), c_G(n_c), c_Gn(n_c);
        std::vector<uint64_t> c_pl_off(n_c), c_out_off(n_c);
        std::vector<uint8_t> c_mono(n_c, 0);
        uint64_t n_pl = 0, n_out = 0;
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i];
            c_call_off[i + 1] = c_call_off[i] + (call_allele_off[e + 1] - call_allele_off[e]);
            c_G[i] = G[e];
            c_Gn[i] = Gn[e];
            c_pl_off[i] = n_pl;
            c_out_off[i] = n_out;
            n_pl += (uint64_t)n_samples * G[e];
            n_out += (uint64_t)n_samples * Gn[e];
            if (site_monomorphic) c_mono[i] = site_monomorphic[e] != 0;
        }
        const uint32_t n_call = c_call_off[n_c];
        std::vector<uint32_t> c_call(n_call);
        std::vector<uint8_t> c_kind(n_call, PHMM_AF_KIND_PLAIN), c_type(n_call, 0);
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i], a0 = event_allele_off[e];
            for (uint32_t c = c_call_off[i]; c < c_call_off[i + 1]; ++c) {
                const uint32_t a = call_allele[call_allele_off[e] + (c - c_call_off[i])];
                c_call[c] = a;
                if (allele_kind) c_kind[c] = allele_kind[a0 + a];
                // calculate_allele_types: the reference; len() == the reference's -> SNP; otherwise INDEL ('*' has length 1)
                if (posteriors) c_type[c] = a == 0 ? 0 : allele_length[a0 + a] == allele_length[a0] ? 1 : 2;
            }
        }

        DevGuard dg(h->device);
        auto &W = h->aswork;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs -----------------------------------------------------------------------------
        size_t o = 0;
        auto place = [&](size_t bytes) {
            const size_t at = o;
            o += up256(bytes);
            return at;
        };
        const size_t n_es = (size_t)n_c * n_samples;
        const size_t o_gc = place(4ull * n_c), o_sc = place(4ull * n_c), o_co = place(4ull * (n_c + 1)), o_ca = place(4ull * n_call),
                     o_kd = place(n_call), o_ty = place(n_call), o_po = place(8ull * n_c), o_pl = place(4ull * n_pl), o_mo = place(n_c),
                     o_to = place(4ull * T.first.size()), o_tc = place(4ull * T.second.size()), o_rk = place(4ull * rank.size()),
                     o_oo = place(8ull * n_c), in_bytes = o;
        const size_t o_pna = place(8ull * n_es);  // device scratch, not copied back
        const size_t o_gp = place(posteriors ? 8ull * n_out : 0), o_pg = place(posteriors ? 8ull * n_out : 0), o_lq = place(8ull * n_es),
                     o_qu = place(8ull * n_c), o_sp = place(4ull * n_out), o_gt = place(4ull * n_es * ploidy), o_gq = place(4ull * n_es),
                     o_cl = place(n_es), o_fl = place(n_es), total = o;
        if (W.cap < total) {
            (void)hipStreamSynchronize(S);
            if (W.dev) (void)hipFree(W.dev);
            if (W.host) (void)hipHostFree(W.host);
            W.dev = W.host = nullptr;
            W.cap = 0;
            const size_t cap = std::max<size_t>(total + total / 2, 1 << 20);
            if (!ok(h, hipMalloc((void **)&W.dev, cap), "hipMalloc(genotype assignment staging)") ||
                !ok(h, hipHostMalloc((void **)&W.host, cap, hipHostMallocDefault), "hipHostMalloc(genotype assignment staging)"))
                return PHMM_ERR_HIP;
            W.cap = cap;
        }
        auto put = [&](size_t at, const void *src, size_t bytes) {
            if (bytes) memcpy(W.host + at, src, bytes);
        };
        put(o_gc, c_G.data(), 4ull * n_c);
        put(o_sc, c_Gn.data(), 4ull * n_c);
        put(o_co, c_call_off.data(), 4ull * (n_c + 1));
        put(o_ca, c_call.data(), 4ull * n_call);
        put(o_kd, c_kind.data(), n_call);
        put(o_ty, c_type.data(), n_call);
        put(o_po, c_pl_off.data(), 8ull * n_c);
        for (uint32_t i = 0; i < n_c; ++i) put(o_pl + 4 * c_pl_off[i], pl + pl_off[computed[i]], 4ull * n_samples * c_G[i]);
        put(o_mo, c_mono.data(), n_c);
        put(o_to, T.first.data(), 4ull * T.first.size());
        put(o_tc, T.second.data(), 4ull * T.second.size());
        put(o_rk, rank.data(), 4ull * rank.size());
        put(o_oo, c_out_off.data(), 8ull * n_c);
        h->stat_staged_bytes += in_bytes;

        AssignParams p{};
        p.n_samples = n_samples;
        p.ploidy = ploidy;
        p.method = posteriors ? AS_USE_POSTERIORS : AS_USE_PLS;
        p.genotype_count = (const uint32_t *)(W.dev + o_gc);
        p.sub_count = (const uint32_t *)(W.dev + o_sc);
        p.call_off = (const uint32_t *)(W.dev + o_co);
        p.call_allele = (const uint32_t *)(W.dev + o_ca);
        p.call_kind = (const uint8_t *)(W.dev + o_kd);
        p.call_type = (const uint8_t *)(W.dev + o_ty);
        p.pl_off = (const uint64_t *)(W.dev + o_po);
        p.pl = (const int32_t *)(W.dev + o_pl);
        p.monomorphic = (const uint8_t *)(W.dev + o_mo);
        p.gt_comp_off = (const uint32_t *)(W.dev + o_to);
        p.gt_comp = (const uint32_t *)(W.dev + o_tc);
        p.rank_off = (const uint32_t *)(W.dev + o_rk);
        p.rank_stride = stride;
        if (posteriors) {
            // GenotypePriorCalculator::assuming_hw with other_het = None (genotype_prior_calculator.rs:46-80, :116-139), by
            // AlleleType ordinal REF, SNP, INDEL, OTHER
            const double log10_snp_norm = std::log10(3.0), other = std::max(log10_snp_het, log10_indel_het);
            const double het[4] = {0.0, log10_snp_het - log10_snp_norm, log10_indel_het, other};
            const double hom[4] = {0.0, log10_snp_het * 2.0 - log10_snp_norm, log10_indel_het * 2.0, other * 2.0};
            for (int k = 0; k < 4; ++k) {
                p.het[k] = het[k];
                p.hom[k] = hom[k];
                p.diff[k] = hom[k] - het[k];
            }
        }
        p.log_10 = std::log(10.0);
        p.inv_log_10 = 1.0 / p.log_10;
        p.log1mexp_threshold = std::log(0.5);
        p.out_off = (const uint64_t *)(W.dev + o_oo);
        p.sub_pl = (int32_t *)(W.dev + o_sp);
        p.gp = (double *)(W.dev + o_gp);
        p.pg = (double *)(W.dev + o_pg);
        p.gt = (int32_t *)(W.dev + o_gt);
        p.gq = (int32_t *)(W.dev + o_gq);
        p.log10_gq = (double *)(W.dev + o_lq);
        p.called = (uint8_t *)(W.dev + o_cl);
        p.flags = (uint8_t *)(W.dev + o_fl);
        p.p_no_alt = (double *)(W.dev + o_pna);
        p.qual_update = (double *)(W.dev + o_qu);
        if (!ok(h, hipMemcpyAsync(W.dev, W.host, in_bytes, hipMemcpyHostToDevice, S), "H2D genotype assignment") ||
            !ok(h, launch_assign(p, n_c, S), "phmm_assign_kernel") ||
            !ok(h, hipMemcpyAsync(W.host + o_gp, W.dev + o_gp, total - o_gp, hipMemcpyDeviceToHost, S), "D2H genotype assignment") ||
            !ok(h, hipStreamSynchronize(S), "sync(genotype assignment)"))
            return PHMM_ERR_HIP;
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i];
            const size_t n = (size_t)n_samples * c_Gn[i], from = c_out_off[i], es = (size_t)e * n_samples, is = (size_t)i * n_samples;
            memcpy(sub_pl + sub_pl_off[e], W.host + o_sp + 4 * from, 4 * n);
            if (posteriors) {
                memcpy(gp + sub_pl_off[e], W.host + o_gp + 8 * from, 8 * n);
                memcpy(pg + sub_pl_off[e], W.host + o_pg + 8 * from, 8 * n);
                log10_p_error_posterior[e] = ((const double *)(W.host + o_qu))[i];
            }
            memcpy(gt + es * ploidy, W.host + o_gt + 4 * is * ploidy, 4ull * n_samples * ploidy);
            memcpy(gq + es, W.host + o_gq + 4 * is, 4ull * n_samples);
            if (log10_gq) memcpy(log10_gq + es, W.host + o_lq + 8 * is, 8ull * n_samples);
            memcpy(sample_called + es, W.host + o_cl + is, n_samples);
            memcpy(sample_flags + es, W.host + o_fl + is, n_samples);
        }
        return PHMM_OK;
    } catch (const std::bad_alloc &) {
        h->err = "phmm_assign_genotypes: out of host memory";
        return h->err_code = PHMM_ERR_NO_MEMORY;
    } catch (const std::exception &e) {
        h->err = std::string("phmm_assign_genotypes: ") + e.what();
        return h->err_code = PHMM_ERR_INTERNAL;
    }
}

}  // extern "C"
