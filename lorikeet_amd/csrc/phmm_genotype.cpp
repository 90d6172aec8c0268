// phmm_genotype_likelihoods (include/phmm.h): host side -- validation, the genotype tables, staging, the resident Jacobian
// table.  The arithmetic runs on the device (phmm_genotype_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "phmm_genotype_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_tables.hpp"

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
    try {
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
        std::vector<uint64_t> lk_off(n_regions, 0);
        uint64_t n_lk = 0;
        for (uint32_t g = 0; g < n_regions; ++g) {
            if (!region_used[g]) continue;
            lk_off[g] = n_lk;
            n_lk += (uint64_t)(region_read_off[g + 1] - region_read_off[g]) * (region_hap_off[g + 1] - region_hap_off[g]);
        }

        // ---- the genotypes of (ploidy, most alleles): the index order of fewer alleles is a prefix of it ------------------
        const auto &T = genotype_table_of(h, ploidy, max_alleles);
        std::vector<double> log10_k(ploidy + 1, 0.0);
        for (uint32_t k = 1; k <= ploidy; ++k) log10_k[k] = std::log10((double)k);

        DevGuard dg(h->device);
        phmm_handle::GtWork &W = h->gwork;
        hipStream_t S = h->streams[0];
        if (!W.d_jacobian) {
            const auto &jac = table_jacobian();
            if (!ok(h, hipMalloc((void **)&W.d_jacobian, jac.size() * sizeof(double)), "hipMalloc(jacobian)") ||
                !ok(h, hipMemcpy(W.d_jacobian, jac.data(), jac.size() * sizeof(double), hipMemcpyHostToDevice), "copy jacobian")) {
                if (W.d_jacobian) (void)hipFree(W.d_jacobian);
                W.d_jacobian = nullptr;
                return PHMM_ERR_HIP;
            }
        }
        // ---- staging: inputs, then [gl | pl | n_evidence] ---------------------------------------------------------------------
        size_t o = 0;
        auto place = [&](size_t bytes) {
            const size_t at = o;
            o += up256(bytes);
            return at;
        };
        const size_t n_gt = T.first.size() - 1;
        const size_t o_rro = place(4ull * (n_regions + 1)), o_rho = place(4ull * (n_regions + 1)), o_lko = place(8ull * n_regions),
                     o_lk = place(8ull * n_lk), o_kp = place(n_reads), o_rs = place(4ull * n_reads), o_st = place(8ull * n_reads),
                     o_en = place(8ull * n_reads), o_er = place(4ull * n_events), o_eao = place(4ull * (n_events + 1)),
                     o_emo = place(4ull * n_events), o_map = place(4ull * n_map), o_es = place(8ull * n_events), o_ee = place(8ull * n_events),
                     o_eoo = place(8ull * n_events), o_gc = place(4ull * n_events), o_co = place(4ull * (n_gt + 1)),
                     o_c = place(4ull * T.second.size()), o_l10 = place(8ull * (ploidy + 1)), in_bytes = o;
        const size_t o_gl = place(8ull * n_out), o_pl = place(4ull * n_out), o_ne = place(4ull * n_events * n_samples), total = o;
        if (W.cap < total) {
            (void)hipStreamSynchronize(S);
            if (W.dev) (void)hipFree(W.dev);
            if (W.host) (void)hipHostFree(W.host);
            W.dev = W.host = nullptr;
            W.cap = 0;
            const size_t cap = std::max<size_t>(total + total / 2, 1 << 20);
            if (!ok(h, hipMalloc((void **)&W.dev, cap), "hipMalloc(genotype staging)") ||
                !ok(h, hipHostMalloc((void **)&W.host, cap, hipHostMallocDefault), "hipHostMalloc(genotype staging)"))
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
        put(o_er, event_region, 4ull * n_events);
        put(o_eao, event_allele_off, 4ull * (n_events + 1));
        put(o_emo, map_off.data(), 4ull * n_events);
        put(o_map, event_hap_allele, 4ull * n_map);
        put(o_es, event_start, 8ull * n_events);
        put(o_ee, event_end, 8ull * n_events);
        put(o_eoo, out_dense.data(), 8ull * n_events);
        put(o_gc, G.data(), 4ull * n_events);
        put(o_co, T.first.data(), 4ull * (n_gt + 1));
        put(o_c, T.second.data(), 4ull * T.second.size());
        put(o_l10, log10_k.data(), 8ull * (ploidy + 1));
        h->stat_staged_bytes += in_bytes;

        GenotypeParams p{};
        p.n_events = n_events;
        p.n_samples = n_samples;
        p.ploidy = ploidy;
        p.region_read_off = (const uint32_t *)(W.dev + o_rro);
        p.region_hap_off = (const uint32_t *)(W.dev + o_rho);
        p.region_lk_off = (const uint64_t *)(W.dev + o_lko);
        p.likelihoods = (const double *)(W.dev + o_lk);
        p.keep = (const uint8_t *)(W.dev + o_kp);
        p.read_sample = (const uint32_t *)(W.dev + o_rs);
        p.read_start = (const int64_t *)(W.dev + o_st);
        p.read_end = (const int64_t *)(W.dev + o_en);
        p.event_region = (const uint32_t *)(W.dev + o_er);
        p.event_allele_off = (const uint32_t *)(W.dev + o_eao);
        p.event_map_off = (const uint32_t *)(W.dev + o_emo);
        p.event_hap_allele = (const int32_t *)(W.dev + o_map);
        p.event_start = (const int64_t *)(W.dev + o_es);
        p.event_end = (const int64_t *)(W.dev + o_ee);
        p.event_out_off = (const uint64_t *)(W.dev + o_eoo);
        p.genotype_count = (const uint32_t *)(W.dev + o_gc);
        p.gt_comp_off = (const uint32_t *)(W.dev + o_co);
        p.gt_comp = (const uint32_t *)(W.dev + o_c);
        p.log10_k = (const double *)(W.dev + o_l10);
        p.jacobian = W.d_jacobian;
        p.gl = (double *)(W.dev + o_gl);
        p.pl = (int32_t *)(W.dev + o_pl);
        p.n_evidence = (uint32_t *)(W.dev + o_ne);
        if (!ok(h, hipMemcpyAsync(W.dev, W.host, in_bytes, hipMemcpyHostToDevice, S), "H2D genotype") ||
            !ok(h, launch_genotype(p, S), "phmm_genotype_kernel") ||
            !ok(h, hipMemcpyAsync(W.host + o_gl, W.dev + o_gl, total - o_gl, hipMemcpyDeviceToHost, S), "D2H genotype") ||
            !ok(h, hipStreamSynchronize(S), "sync(genotype)"))
            return PHMM_ERR_HIP;
        for (uint32_t e = 0; e < n_events; ++e) {
            const size_t n = (size_t)n_samples * G[e];
            memcpy(gl + gl_off[e], W.host + o_gl + 8 * out_dense[e], 8 * n);
            if (pl) memcpy(pl + gl_off[e], W.host + o_pl + 4 * out_dense[e], 4 * n);
        }
        if (n_evidence) memcpy(n_evidence, W.host + o_ne, 4ull * n_events * n_samples);
        return PHMM_OK;
    } catch (const std::bad_alloc &) {
        h->err = "phmm_genotype_likelihoods: out of host memory";
        return h->err_code = PHMM_ERR_NO_MEMORY;
    } catch (const std::exception &e) {
        h->err = std::string("phmm_genotype_likelihoods: ") + e.what();
        return h->err_code = PHMM_ERR_INTERNAL;
    }
}

}  // extern "C"
