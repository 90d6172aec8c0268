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
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

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
    PHMM_GUARD_BEGIN
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
        std::vector<uint64_t> c_out_off(n_c);
        std::vector<uint8_t> c_mono(n_c, 0);
        uint64_t n_out = 0;
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i];
            c_call_off[i + 1] = c_call_off[i] + (call_allele_off[e + 1] - call_allele_off[e]);
            c_G[i] = G[e];
            c_Gn[i] = Gn[e];
            c_out_off[i] = n_out;
            n_out += (uint64_t)n_samples * Gn[e];
            if (site_monomorphic) c_mono[i] = site_monomorphic[e] != 0;
        }
        const DensePls pls(computed, c_G, n_samples);
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

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->assign_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs -----------------------------------------------------------------------------
        const size_t n_es = (size_t)n_c * n_samples;
        StageLayout L;
        const auto s_gc = L.in(c_G.data(), n_c), s_sc = L.in(c_Gn.data(), n_c), s_co = L.in(c_call_off.data(), n_c + 1), s_ca = L.in(c_call.data(), n_call);
        const auto s_kd = L.in(c_kind.data(), n_call), s_ty = L.in(c_type.data(), n_call);
        const auto s_po = L.in(pls.off.data(), n_c);
        const auto s_pl = L.in<int32_t>(pls.n);  // packed below
        const auto s_mo = L.in(c_mono.data(), n_c);
        const auto s_to = L.in(T.first.data(), T.first.size()), s_tc = L.in(T.second.data(), T.second.size()), s_rk = L.in(rank.data(), rank.size());
        const auto s_oo = L.in(c_out_off.data(), n_c);
        L.end_inputs();
        const auto s_pna = L.scratch<double>(n_es);
        const auto s_gp = L.out<double>(posteriors ? n_out : 0), s_pg = L.out<double>(posteriors ? n_out : 0), s_lq = L.out<double>(n_es), s_qu = L.out<double>(n_c);
        const auto s_sp = L.out<int32_t>(n_out), s_gt = L.out<int32_t>(n_es * ploidy), s_gq = L.out<int32_t>(n_es);
        const auto s_cl = L.out<uint8_t>(n_es), s_fl = L.out<uint8_t>(n_es);
        if (!W.reserve(h, L, "genotype assignment staging")) return PHMM_ERR_HIP;
        pls.into(W.host_ptr(s_pl), pl_off, pl);
        h->stat_staged_bytes += L.in_bytes;

        AssignParams p{};
        p.n_samples = n_samples;
        p.ploidy = ploidy;
        p.method = posteriors ? AS_USE_POSTERIORS : AS_USE_PLS;
        p.genotype_count = W.dev_ptr(s_gc);
        p.sub_count = W.dev_ptr(s_sc);
        p.call_off = W.dev_ptr(s_co);
        p.call_allele = W.dev_ptr(s_ca);
        p.call_kind = W.dev_ptr(s_kd);
        p.call_type = W.dev_ptr(s_ty);
        p.pl_off = W.dev_ptr(s_po);
        p.pl = W.dev_ptr(s_pl);
        p.monomorphic = W.dev_ptr(s_mo);
        p.gt_comp_off = W.dev_ptr(s_to);
        p.gt_comp = W.dev_ptr(s_tc);
        p.rank_off = W.dev_ptr(s_rk);
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
        p.out_off = W.dev_ptr(s_oo);
        p.sub_pl = W.dev_ptr(s_sp);
        p.gp = W.dev_ptr(s_gp);
        p.pg = W.dev_ptr(s_pg);
        p.gt = W.dev_ptr(s_gt);
        p.gq = W.dev_ptr(s_gq);
        p.log10_gq = W.dev_ptr(s_lq);
        p.called = W.dev_ptr(s_cl);
        p.flags = W.dev_ptr(s_fl);
        p.p_no_alt = W.dev_ptr(s_pna);
        p.qual_update = W.dev_ptr(s_qu);
        if (!stage_round_trip(h, W, L, S, "genotype assignment", [&] { return hip_ok(h, launch_assign(p, n_c, S), "phmm_assign_kernel"); })) return PHMM_ERR_HIP;
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i];
            const size_t n = (size_t)n_samples * c_Gn[i], from = c_out_off[i], es = (size_t)e * n_samples, is = (size_t)i * n_samples;
            memcpy(sub_pl + sub_pl_off[e], W.host_ptr(s_sp) + from, 4 * n);
            if (posteriors) {
                memcpy(gp + sub_pl_off[e], W.host_ptr(s_gp) + from, 8 * n);
                memcpy(pg + sub_pl_off[e], W.host_ptr(s_pg) + from, 8 * n);
                log10_p_error_posterior[e] = W.host_ptr(s_qu)[i];
            }
            memcpy(gt + es * ploidy, W.host_ptr(s_gt) + is * ploidy, 4ull * n_samples * ploidy);
            memcpy(gq + es, W.host_ptr(s_gq) + is, 4ull * n_samples);
            if (log10_gq) memcpy(log10_gq + es, W.host_ptr(s_lq) + is, 8ull * n_samples);
            memcpy(sample_called + es, W.host_ptr(s_cl) + is, n_samples);
            memcpy(sample_flags + es, W.host_ptr(s_fl) + is, n_samples);
        }
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assign_genotypes", PHMM_FAIL_CODE)
}

}  // extern "C"
