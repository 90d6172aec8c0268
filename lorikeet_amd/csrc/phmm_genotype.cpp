// phmm_genotype_likelihoods (include/phmm.h): host side -- validation, the genotype tables, staging, the resident Jacobian
// table.  The arithmetic runs on the device (phmm_genotype_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "phmm_genotype_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"
#include "phmm_tables.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_genotype_likelihoods: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

constexpr uint32_t kMaxPloidy = 65535;  // (a genotype's allele counts are 16-bit in the kernel's table)

// The genotypes of (ploidy, n_alleles) in the reference's index order (allele_heap_to_index, genotype_likelihood_calculator.rs:
// 273-295: the sorted alleles a_1 <= ... <= a_p sit at sum offset[i][a_i]); each as its distinct alleles, ascending, with
// their counts (GenotypeAlleleCounts).  Only called with genotype_count(ploidy, n_alleles) <= GT_MAX_GENOTYPES.
void genotype_table(uint32_t ploidy, uint32_t n_alleles, std::vector<uint32_t> *comp_off, std::vector<uint32_t> *comp) {
    const auto off = genotype_offset_table(ploidy, n_alleles);
    const uint32_t G = (uint32_t)off[ploidy][n_alleles];
    std::vector<std::vector<uint32_t>> by_index(G);
    std::vector<uint32_t> counts(n_alleles, 0);
    // every vector of allele counts summing to the ploidy
    auto visit = [&](auto &&self, uint32_t a, uint32_t remaining) -> void {
        if (a + 1 == n_alleles) {
            counts[a] = remaining;
            uint64_t index = 0;
            uint32_t i = 1;
            std::vector<uint32_t> c;
            for (uint32_t b = 0; b < n_alleles; ++b) {
                for (uint32_t k = 0; k < counts[b]; ++k) index += off[i++][b];
                if (counts[b]) c.push_back(b | counts[b] << 16);
            }
            by_index[index] = std::move(c);
            return;
        }
        for (uint32_t k = 0; k <= remaining; ++k) {
            counts[a] = k;
            self(self, a + 1, remaining - k);
        }
    };
    visit(visit, 0, ploidy);
    comp_off->assign(1, 0);
    comp->clear();
    for (const auto &c : by_index) {
        comp->insert(comp->end(), c.begin(), c.end());
        comp_off->push_back((uint32_t)comp->size());
    }
}

}  // namespace

std::vector<std::vector<uint64_t>> genotype_offset_table(uint32_t ploidy, uint32_t n_alleles) {
    std::vector<std::vector<uint64_t>> off(ploidy + 1, std::vector<uint64_t>(n_alleles + 1, 0));
    for (uint32_t a = 1; a <= n_alleles; ++a) off[0][a] = 1;
    for (uint32_t p = 1; p <= ploidy; ++p)
        for (uint32_t a = 1; a <= n_alleles; ++a) off[p][a] = std::min<uint64_t>(off[p][a - 1] + off[p - 1][a], UINT32_MAX);
    return off;
}

const std::pair<std::vector<uint32_t>, std::vector<uint32_t>> &genotype_table_of(phmm_handle *h, uint32_t ploidy, uint32_t n_alleles) {
    auto &T = h->gwork.tables[(uint64_t)ploidy << 32 | n_alleles];
    if (T.first.empty()) genotype_table(ploidy, n_alleles, &T.first, &T.second);
    return T;
}

extern "C" {

uint32_t phmm_genotype_count(uint32_t ploidy, uint32_t n_alleles) {
    // C(ploidy + n_alleles - 1, k), k = min(ploidy, n_alleles - 1): C(n, i) grows with i up to k <= n / 2, so the first
    // partial product past UINT32_MAX means the count saturates
    if (!ploidy || !n_alleles) return 0;
    const uint64_t n = (uint64_t)ploidy + n_alleles - 1, k = std::min<uint64_t>(ploidy, n_alleles - 1);
    unsigned __int128 c = 1;
    for (uint64_t i = 1; i <= k; ++i) {
        c = c * (n - k + i) / i;
        if (c > UINT32_MAX) return UINT32_MAX;
    }
    return (uint32_t)c;
}

size_t phmm_table_jacobian(const double **table) {
    *table = table_jacobian().data();
    return table_jacobian().size();
}

int phmm_genotype_likelihoods(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                              const uint64_t *out_off, const double *likelihoods, const uint8_t *keep, const uint32_t *read_sample,
                              const int64_t *read_start, const int64_t *read_end, uint32_t n_samples, uint32_t ploidy,
                              uint32_t n_events, const uint32_t *event_region, const uint32_t *event_allele_off,
                              const int64_t *event_start, const int64_t *event_end, const int32_t *event_hap_allele,
                              const uint64_t *gl_off, double *gl, int32_t *pl, uint32_t *n_evidence) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        if (!n_events) return PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!region_read_off || !region_hap_off || !out_off || !likelihoods || !event_region || !event_allele_off || !event_start ||
            !event_end || !event_hap_allele || !gl_off || !gl)
            return fail(h, "null array");
        if (!ploidy) return fail(h, "ploidy must be at least 1");
        if (ploidy > kMaxPloidy) return fail(h, "ploidy beyond " + std::to_string(kMaxPloidy));
        if (region_read_off[0] != 0 || region_hap_off[0] != 0) return fail(h, "region offset arrays must start at 0");
        for (uint32_t g = 0; g < n_regions; ++g)
            if (region_read_off[g + 1] < region_read_off[g] || region_hap_off[g + 1] < region_hap_off[g])
                return fail(h, "region offsets not monotonic at region " + std::to_string(g));
        const uint32_t n_reads = n_regions ? region_read_off[n_regions] : 0;
        if (n_reads && (!read_sample || !read_start || !read_end)) return fail(h, "null array");
        for (uint32_t r = 0; r < n_reads; ++r)
            if (read_sample[r] >= n_samples) return fail(h, "read " + std::to_string(r) + ": read_sample outside [0, n_samples)");
        std::vector<uint32_t> G(n_events), map_off(n_events);
        std::vector<uint64_t> out_dense(n_events);
        std::vector<char> region_used(n_regions, 0);
        uint64_t n_map = 0, n_out = 0;
        uint32_t max_alleles = 0;
        for (uint32_t e = 0; e < n_events; ++e) {
            const std::string ev = "event " + std::to_string(e) + ": ";
            if (event_region[e] >= n_regions) return fail(h, ev + "event_region outside [0, n_regions)");
            if (event_allele_off[e + 1] < event_allele_off[e]) return fail(h, ev + "event_allele_off not monotonic");
            const uint32_t A = event_allele_off[e + 1] - event_allele_off[e];
            if (!A) return fail(h, ev + "no alleles");
            G[e] = phmm_genotype_count(ploidy, A);
            if (G[e] > GT_MAX_GENOTYPES)
                return fail(h, ev + std::to_string(G[e]) + " genotypes, more than " + std::to_string(GT_MAX_GENOTYPES));
            const uint32_t g = event_region[e], nh = region_hap_off[g + 1] - region_hap_off[g];
            for (uint32_t k = 0; k < nh; ++k) {
                const int32_t a = event_hap_allele[n_map + k];
                if (a < -1 || a >= (int32_t)A) return fail(h, ev + "haplotype " + std::to_string(k) + " maps outside [-1, A_e)");
            }
            if (gl_off[e + 1] < gl_off[e] || gl_off[e + 1] - gl_off[e] < (uint64_t)n_samples * G[e])
                return fail(h, ev + "gl_off slot smaller than n_samples x genotypes");
            if (n_map > UINT32_MAX) return fail(h, "haplotype -> allele maps beyond 2^32 entries");
            map_off[e] = (uint32_t)n_map;
            n_map += nh;
            out_dense[e] = n_out;
            n_out += (uint64_t)n_samples * G[e];
            region_used[g] = 1;
            max_alleles = std::max(max_alleles, A);
        }
        const LikelihoodGather lks(n_regions, region_read_off, region_hap_off, region_used);

        // ---- the genotypes of (ploidy, most alleles): the index order of fewer alleles is a prefix of it ------------------
        const auto &T = genotype_table_of(h, ploidy, max_alleles);
        std::vector<double> log10_k(ploidy + 1, 0.0);
        for (uint32_t k = 1; k <= ploidy; ++k) log10_k[k] = std::log10((double)k);

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->gwork.staging;
        hipStream_t S = h->streams[0];
        if (!h->gwork.d_jacobian) {
            const auto &jac = table_jacobian();
            double *&d_jac = h->gwork.d_jacobian;
            if (!hip_ok(h, hipMalloc((void **)&d_jac, jac.size() * sizeof(double)), "hipMalloc(jacobian)") ||
                !hip_ok(h, hipMemcpy(d_jac, jac.data(), jac.size() * sizeof(double), hipMemcpyHostToDevice), "copy jacobian")) {
                if (d_jac) (void)hipFree(d_jac);
                d_jac = nullptr;
                return PHMM_ERR_HIP;
            }
        }
        // ---- staging: inputs, then [gl | pl | n_evidence] ---------------------------------------------------------------------
        StageLayout L;
        const auto s_rro = L.in(region_read_off, n_regions + 1), s_rho = L.in(region_hap_off, n_regions + 1);
        const auto s_lko = L.in(lks.off.data(), n_regions);
        const auto s_lk = L.in<double>(lks.n);
        const auto s_kp = L.in<uint8_t>(n_reads);
        const auto s_rs = L.in(read_sample, n_reads);
        const auto s_st = L.in(read_start, n_reads), s_en = L.in(read_end, n_reads);
        const auto s_er = L.in(event_region, n_events), s_eao = L.in(event_allele_off, n_events + 1), s_emo = L.in(map_off.data(), n_events);
        const auto s_map = L.in(event_hap_allele, n_map);
        const auto s_es = L.in(event_start, n_events), s_ee = L.in(event_end, n_events);
        const auto s_eoo = L.in(out_dense.data(), n_events);
        const auto s_gc = L.in(G.data(), n_events), s_co = L.in(T.first.data(), T.first.size()), s_c = L.in(T.second.data(), T.second.size());
        const auto s_l10 = L.in(log10_k.data(), ploidy + 1);
        L.end_inputs();
        const auto s_gl = L.out<double>(n_out);
        const auto s_pl = L.out<int32_t>(n_out);
        const auto s_ne = L.out<uint32_t>((size_t)n_events * n_samples);
        if (!W.reserve(h, L, "genotype staging")) return PHMM_ERR_HIP;
        lks.into(W.host_ptr(s_lk), W.host_ptr(s_kp), out_off, likelihoods, keep);
        h->stat_staged_bytes += L.in_bytes;

        GenotypeParams p{};
        p.n_events = n_events;
        p.n_samples = n_samples;
        p.ploidy = ploidy;
        p.region_read_off = W.dev_ptr(s_rro);
        p.region_hap_off = W.dev_ptr(s_rho);
        p.region_lk_off = W.dev_ptr(s_lko);
        p.likelihoods = W.dev_ptr(s_lk);
        p.keep = W.dev_ptr(s_kp);
        p.read_sample = W.dev_ptr(s_rs);
        p.read_start = W.dev_ptr(s_st);
        p.read_end = W.dev_ptr(s_en);
        p.event_region = W.dev_ptr(s_er);
        p.event_allele_off = W.dev_ptr(s_eao);
        p.event_map_off = W.dev_ptr(s_emo);
        p.event_hap_allele = W.dev_ptr(s_map);
        p.event_start = W.dev_ptr(s_es);
        p.event_end = W.dev_ptr(s_ee);
        p.event_out_off = W.dev_ptr(s_eoo);
        p.genotype_count = W.dev_ptr(s_gc);
        p.gt_comp_off = W.dev_ptr(s_co);
        p.gt_comp = W.dev_ptr(s_c);
        p.log10_k = W.dev_ptr(s_l10);
        p.jacobian = h->gwork.d_jacobian;
        p.gl = W.dev_ptr(s_gl);
        p.pl = W.dev_ptr(s_pl);
        p.n_evidence = W.dev_ptr(s_ne);
        if (!stage_round_trip(h, W, L, S, "genotype", [&] { return hip_ok(h, launch_genotype(p, S), "phmm_genotype_kernel"); })) return PHMM_ERR_HIP;
        for (uint32_t e = 0; e < n_events; ++e) {
            const size_t n = (size_t)n_samples * G[e];
            memcpy(gl + gl_off[e], W.host_ptr(s_gl) + out_dense[e], 8 * n);
            if (pl) memcpy(pl + gl_off[e], W.host_ptr(s_pl) + out_dense[e], 4 * n);
        }
        if (n_evidence) memcpy(n_evidence, W.host_ptr(s_ne), 4ull * n_events * n_samples);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_genotype_likelihoods", PHMM_FAIL_CODE)
}

}  // extern "C"
