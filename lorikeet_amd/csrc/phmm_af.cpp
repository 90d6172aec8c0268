// phmm_allele_frequency (include/phmm.h): host side -- validation, prior classes, the genotype tables with their log10
// combination counts, staging.  The arithmetic runs on the device (phmm_af_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "phmm_af_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_allele_frequency: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

// MathUtils::log10_factorial (math_utils.rs:133-135): ln_gamma(n + 1) * LOG10_E
double log10_factorial(double n) { return std::lgamma(n + 1.0) * std::log10(M_E); }

uint32_t genotypes_per_lane(uint32_t G) { return af_genotypes_per_lane(G); }

}  // namespace

namespace phmm {

uint32_t af_genotypes_per_lane(uint32_t G) { return G <= 64 ? 1 : G <= 256 ? 4 : G <= 512 ? 8 : 16; }

bool af_is_block_event(uint32_t G, uint32_t n_samples) {
    uint32_t S = 64;
    if (af_genotypes_per_lane(G) == 1) {
        S = 1;
        while (S < G) S <<= 1;
    }
    return (n_samples + 64 / S - 1) / (64 / S) >= AF_BLOCK_PASSES;
}

AfGenotypeTables af_genotype_tables(const std::pair<std::vector<uint32_t>, std::vector<uint32_t>> &T, uint32_t ploidy) {
    AfGenotypeTables t;
    const size_t n_gt = T.first.size() - 1;
    t.log10_comb.resize(n_gt);
    t.gt_alleles.assign(n_gt, 0);
    const double log10_ploidy_factorial = log10_factorial((double)ploidy);
    for (size_t g = 0; g < n_gt; ++g) {
        double s = 0.0;
        for (uint32_t c = T.first[g]; c < T.first[g + 1]; ++c) {
            s += log10_factorial((double)(T.second[c] >> 16));
            t.gt_alleles[g] |= 1ull << (T.second[c] & 0xffffu);
        }
        t.log10_comb[g] = log10_ploidy_factorial - s;  // GenotypeAlleleCounts::log10_combination_count
    }
    t.neg_log10_alleles.assign(AF_MAX_ALLELES + 1, 0.0);
    for (uint32_t a = 1; a <= AF_MAX_ALLELES; ++a) t.neg_log10_alleles[a] = -std::log10((double)a);
    return t;
}

}  // namespace phmm

extern "C" {

int phmm_allele_frequency(phmm_handle *h, uint32_t n_events, uint32_t n_samples, uint32_t ploidy, const uint32_t *event_allele_off,
                          const uint32_t *allele_length, const uint8_t *allele_kind, const uint64_t *pl_off, const int32_t *pl,
                          double ref_pseudo_count, double snp_pseudo_count, double indel_pseudo_count, double stand_min_conf,
                          double *log10_p_no_variant, double *log10_p_variant_present, double *log10_p_absent, int64_t *mle_count,
                          uint8_t *allele_flags, double *qual, uint32_t *flags, uint32_t *iterations) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        if (!n_events) return PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!event_allele_off || !allele_length || !pl_off || !log10_p_no_variant || !log10_p_variant_present ||
            !log10_p_absent || !mle_count || !qual || !flags)
            return fail(h, "null array");
        if (!ploidy) return fail(h, "ploidy must be at least 1");
        if (n_samples && !pl) return fail(h, "null array");
        std::vector<uint32_t> computed, G(n_events, 0);
        std::vector<int32_t> span_del(n_events, -1);
        uint32_t max_alleles = 0;
        for (uint32_t e = 0; e < n_events; ++e) {
            const std::string ev = "event " + std::to_string(e) + ": ";
            if (event_allele_off[e + 1] < event_allele_off[e]) return fail(h, ev + "event_allele_off not monotonic");
            if (pl_off[e + 1] < pl_off[e]) return fail(h, ev + "pl_off not monotonic");
            const uint32_t a0 = event_allele_off[e], A = event_allele_off[e + 1] - a0;
            if (A < 2) return fail(h, ev + "fewer than 2 alleles");
            if (allele_kind) {
                if (allele_kind[a0] != PHMM_AF_KIND_PLAIN) return fail(h, ev + "allele 0 (the reference) is not plain");
                for (uint32_t a = 1; a < A; ++a) {
                    const uint8_t k = allele_kind[a0 + a];
                    if (k > PHMM_AF_KIND_NON_REF) return fail(h, ev + "allele " + std::to_string(a) + ": unknown kind");
                    if (k == PHMM_AF_KIND_SPAN_DEL) {
                        if (span_del[e] >= 0) return fail(h, ev + "more than one '*' allele");
                        span_del[e] = (int32_t)a;
                    }
                }
            }
            if (A > AF_MAX_ALLELES) continue;  // PHMM_AF_TOO_MANY_ALLELES: not called, no genotypes enumerated
            G[e] = phmm_genotype_count(ploidy, A);
            if (G[e] > AF_MAX_GENOTYPES)
                return fail(h, ev + std::to_string(G[e]) + " genotypes, more than " + std::to_string(AF_MAX_GENOTYPES));
            if (pl_off[e + 1] - pl_off[e] < (uint64_t)n_samples * G[e]) return fail(h, ev + "pl_off slot smaller than n_samples x genotypes");
            if (n_samples) {
                computed.push_back(e);
                max_alleles = std::max(max_alleles, A);
            }
        }

        // ---- events that are not computed: too many alleles, or no samples -------------------------------------------------
        for (uint32_t e = 0; e < n_events; ++e) {
            const uint32_t A = event_allele_off[e + 1] - event_allele_off[e];
            if (A <= AF_MAX_ALLELES && n_samples) continue;
            log10_p_no_variant[e] = log10_p_variant_present[e] = qual[e] = 0.0;
            flags[e] = A > AF_MAX_ALLELES ? PHMM_AF_TOO_MANY_ALLELES : 0u;
            if (iterations) iterations[e] = 0;
            for (uint32_t a = event_allele_off[e]; a < event_allele_off[e + 1]; ++a) {
                log10_p_absent[a] = 0.0;
                mle_count[a] = 0;
                if (allele_flags) allele_flags[a] = 0;
            }
        }
        const uint32_t n_c = (uint32_t)computed.size();
        if (!n_c) return PHMM_OK;

        // ---- the genotypes of (ploidy, most alleles): the index order of fewer alleles is a prefix of it ------------------
        const auto &T = genotype_table_of(h, ploidy, max_alleles);
        const size_t n_gt = T.first.size() - 1;
        const AfGenotypeTables GT = af_genotype_tables(T, ploidy);
        const std::vector<double> &log10_comb = GT.log10_comb, &neg_log10_alleles = GT.neg_log10_alleles;
        const std::vector<uint64_t> &gt_alleles = GT.gt_alleles;

        // ---- the computed events, densely: alleles with their prior pseudo counts, PLs ------------------------------------
        std::vector<uint32_t> c_allele_off(n_c + 1, 0), c_G(n_c);
        std::vector<int32_t> c_span_del(n_c);
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i];
            c_allele_off[i + 1] = c_allele_off[i] + (event_allele_off[e + 1] - event_allele_off[e]);
            c_G[i] = G[e];
            c_span_del[i] = span_del[e];
        }
        const DensePls pls(computed, c_G, n_samples);
        const uint32_t n_al = c_allele_off[n_c];
        std::vector<double> prior(n_al);
        std::vector<uint8_t> kind(n_al, PHMM_AF_KIND_PLAIN);
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i], a0 = event_allele_off[e], A = c_allele_off[i + 1] - c_allele_off[i];
            for (uint32_t a = 0; a < A; ++a) {
                // allele_frequency_calculator.rs:205-217: reference; length of the reference -> SNP; otherwise indel
                prior[c_allele_off[i] + a] = a == 0                                  ? ref_pseudo_count
                                             : allele_length[a0 + a] == allele_length[a0] ? snp_pseudo_count
                                                                                          : indel_pseudo_count;
                if (allele_kind) kind[c_allele_off[i] + a] = allele_kind[a0 + a];
            }
        }
        // the work lists: per genotypes-per-lane class, first the events of one wave, then the events of a workgroup
        std::vector<uint32_t> work;
        uint32_t cls_off[4][3] = {};  // [class][wave begin, wave count, block count]
        const uint32_t classes[4] = {1, 4, 8, 16};
        for (int c = 0; c < 4; ++c) {
            cls_off[c][0] = (uint32_t)work.size();
            for (int block = 0; block < 2; ++block) {
                for (uint32_t i = 0; i < n_c; ++i) {
                    if (genotypes_per_lane(c_G[i]) != classes[c]) continue;
                    if (af_is_block_event(c_G[i], n_samples) == (block == 1)) work.push_back(i);
                }
                cls_off[c][1 + block] = (uint32_t)work.size() - cls_off[c][0] - (block ? cls_off[c][1] : 0);
            }
        }

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->af_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs -----------------------------------------------------------------------------
        StageLayout L;
        const auto s_wk = L.in(work.data(), work.size()), s_ao = L.in(c_allele_off.data(), n_c + 1), s_gc = L.in(c_G.data(), n_c);
        const auto s_sd = L.in(c_span_del.data(), n_c);
        const auto s_po = L.in(pls.off.data(), n_c);
        const auto s_pl = L.in<int32_t>(pls.n);  // packed below
        const auto s_pr = L.in(prior.data(), n_al);
        const auto s_kd = L.in(kind.data(), n_al);
        const auto s_co = L.in(T.first.data(), T.first.size()), s_c = L.in(T.second.data(), T.second.size());
        const auto s_lc = L.in(log10_comb.data(), n_gt);
        const auto s_ga = L.in(gt_alleles.data(), n_gt);
        const auto s_nl = L.in(neg_log10_alleles.data(), AF_MAX_ALLELES + 1);
        L.end_inputs();
        const auto s_pnv = L.out<double>(n_c), s_pvp = L.out<double>(n_c), s_q = L.out<double>(n_c);
        const auto s_fl = L.out<uint32_t>(n_c), s_it = L.out<uint32_t>(n_c);
        const auto s_abs = L.out<double>(n_al);
        const auto s_mle = L.out<int64_t>(n_al);
        const auto s_af = L.out<uint8_t>(n_al);
        if (!W.reserve(h, L, "allele-frequency staging")) return PHMM_ERR_HIP;
        pls.into(W.host_ptr(s_pl), pl_off, pl);
        h->stat_staged_bytes += L.in_bytes;

        AfParams p{};
        p.n_samples = n_samples;
        p.allele_off = W.dev_ptr(s_ao);
        p.genotype_count = W.dev_ptr(s_gc);
        p.span_del = W.dev_ptr(s_sd);
        p.pl_off = W.dev_ptr(s_po);
        p.pl = W.dev_ptr(s_pl);
        p.prior = W.dev_ptr(s_pr);
        p.kind = W.dev_ptr(s_kd);
        p.gt_comp_off = W.dev_ptr(s_co);
        p.gt_comp = W.dev_ptr(s_c);
        p.gt_log10_comb = W.dev_ptr(s_lc);
        p.gt_alleles = W.dev_ptr(s_ga);
        p.neg_log10_alleles = W.dev_ptr(s_nl);
        p.stand_min_conf = stand_min_conf;
        p.log_10 = std::log(10.0);
        p.inv_log_10 = 1.0 / p.log_10;
        p.log1mexp_threshold = std::log(0.5);
        p.log10_p_no_variant = W.dev_ptr(s_pnv);
        p.log10_p_variant_present = W.dev_ptr(s_pvp);
        p.qual = W.dev_ptr(s_q);
        p.flags = W.dev_ptr(s_fl);
        p.iterations = W.dev_ptr(s_it);
        p.log10_p_absent = W.dev_ptr(s_abs);
        p.mle_count = W.dev_ptr(s_mle);
        p.allele_flags = W.dev_ptr(s_af);
        if (!stage_upload(h, W, L, S, "allele frequency")) return PHMM_ERR_HIP;
        for (int c = 0; c < 4; ++c) {
            p.work = W.dev_ptr(s_wk) + cls_off[c][0];
            p.n_wave_events = cls_off[c][1];
            p.n_block_events = cls_off[c][2];
            if (!hip_ok(h, launch_af(p, classes[c], S), "phmm_af_kernel")) return PHMM_ERR_HIP;
        }
        if (!stage_download(h, W, L, S, "allele frequency")) return PHMM_ERR_HIP;
        const double *r_pnv = W.host_ptr(s_pnv), *r_pvp = W.host_ptr(s_pvp), *r_q = W.host_ptr(s_q), *r_abs = W.host_ptr(s_abs);
        const uint32_t *r_fl = W.host_ptr(s_fl), *r_it = W.host_ptr(s_it);
        const int64_t *r_mle = W.host_ptr(s_mle);
        const uint8_t *r_af = W.host_ptr(s_af);
        for (uint32_t i = 0; i < n_c; ++i) {
            const uint32_t e = computed[i], a0 = event_allele_off[e], c0 = c_allele_off[i], A = c_allele_off[i + 1] - c0;
            log10_p_no_variant[e] = r_pnv[i];
            log10_p_variant_present[e] = r_pvp[i];
            qual[e] = r_q[i];
            flags[e] = r_fl[i];
            if (iterations) iterations[e] = r_it[i];
            memcpy(log10_p_absent + a0, r_abs + c0, 8ull * A);
            memcpy(mle_count + a0, r_mle + c0, 8ull * A);
            if (allele_flags) memcpy(allele_flags + a0, r_af + c0, A);
        }
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_allele_frequency", PHMM_FAIL_CODE)
}

}  // extern "C"
