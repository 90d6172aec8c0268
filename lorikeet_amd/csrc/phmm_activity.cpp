// phmm_activity_profile (include/phmm.h): host side -- validation, the walk over the CIGARs that sizes the workspace and finds
// the windows the reference would panic on, the read-range index, the host-made tables, staging.  The pileup, the sums, the
// allele-frequency step and the band-pass run on the device (phmm_activity_kernels.hip, phmm_af_kernels.hip); there is no CPU
// path here.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phmm_activity_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"
#include "phmm_tables.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_activity_profile: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

constexpr double kMinProbToKeepInFilter = 1e-5;  // BandPassActivityProfile::MIN_PROB_TO_KEEP_IN_FILTER

// BandPassActivityProfile::new (band_pass_activity_profile.rs:36-67): the filter size and its kernel; false where the
// reference's assertions fail (a negative sigma, a sum that is not >= 0)
bool band_kernel(uint32_t max_filter_size, double sigma, bool adaptive, uint32_t *filter_size, std::vector<double> *kernel) {
    if (!(sigma >= 0.0)) return false;
    uint32_t F = max_filter_size;
    if (adaptive) {
        const std::vector<double> full = activity_gaussian_kernel(max_filter_size, sigma);
        if (full.empty()) return false;
        F = activity_filter_size(full, kMinProbToKeepInFilter);
    }
    *kernel = activity_gaussian_kernel(F, sigma);
    *filter_size = F;
    return !kernel->empty();
}

}  // namespace

extern "C" {

int phmm_activity_band_kernel(uint32_t max_filter_size, double sigma, int adaptive_filter_size, uint32_t *filter_size, double *kernel) {
    if (!filter_size || max_filter_size > PHMM_ACTIVITY_MAX_FILTER) return PHMM_ERR_INVALID_ARG;
    try {
        std::vector<double> k;
        if (!band_kernel(max_filter_size, sigma, adaptive_filter_size != 0, filter_size, &k)) return PHMM_ERR_INVALID_ARG;
        if (kernel) std::copy(k.begin(), k.end(), kernel);
    } catch (...) {
        return PHMM_ERR_NO_MEMORY;
    }
    return PHMM_OK;
}

int phmm_activity_term_table(uint32_t ploidy, double *term) {
    if (!term || !ploidy || ploidy > ACT_MAX_PLOIDY) return PHMM_ERR_INVALID_ARG;
    try {
        const std::vector<double> t = activity_term_table(ploidy);
        std::copy(t.begin(), t.end(), term);
    } catch (...) {
        return PHMM_ERR_NO_MEMORY;
    }
    return PHMM_OK;
}

int phmm_activity_profile(phmm_handle *h, uint32_t n_windows, uint32_t n_samples, uint32_t ploidy, uint32_t min_base_quality,
                          double ref_pseudo_count, double snp_pseudo_count, double indel_pseudo_count, double stand_min_conf,
                          uint32_t max_prob_propagation, uint32_t max_filter_size, double sigma, int adaptive_filter_size,
                          uint32_t profile_size, const uint64_t *window_start, const uint32_t *window_len,
                          const uint64_t *window_contig_length, const uint32_t *window_ref_off, const uint8_t *ref_bases,
                          const uint32_t *group_read_off, const int64_t *read_pos, const uint32_t *read_cigar_off,
                          const uint32_t *read_cigar, const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *read_quals,
                          int32_t *window_status, uint32_t *read_counts, uint32_t *ref_depth, uint32_t *non_ref_depth, double *gl,
                          int32_t *pl, double *soft_clip_mean, uint32_t *soft_clip_count, double *qual, uint32_t *af_flags,
                          void *is_active_prob, uint32_t *filter_size, void *profile_prob, uint32_t *profile_len) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        (void)snp_pseudo_count;  // the symbolic alternate allele is never of the reference allele's length
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!ploidy || ploidy > ACT_MAX_PLOIDY)
            return fail(h, "ploidy " + std::to_string(ploidy) + " is outside 1..=" + std::to_string(ACT_MAX_PLOIDY));
        if (!n_samples) return fail(h, "no samples");
        if (max_filter_size > PHMM_ACTIVITY_MAX_FILTER)
            return fail(h, "max_filter_size " + std::to_string(max_filter_size) + " is more than " + std::to_string(PHMM_ACTIVITY_MAX_FILTER));
        uint32_t F = 0;
        std::vector<double> kernel;
        if (!band_kernel(max_filter_size, sigma, adaptive_filter_size != 0, &F, &kernel))
            return fail(h, "sigma gives no Gaussian kernel (negative, or the taps do not sum to a number >= 0)");
        if (!n_windows) {
            if (filter_size) *filter_size = F;
            return PHMM_OK;
        }
        if (!window_start || !window_len || !window_contig_length || !window_ref_off || !group_read_off || !window_status)
            return fail(h, "null array");
        if (window_ref_off[0]) return fail(h, "window_ref_off does not start at 0");
        if (group_read_off[0]) return fail(h, "group_read_off does not start at 0");
        const uint64_t n_groups = (uint64_t)n_windows * n_samples;
        if (n_groups >> 31) return fail(h, "windows x samples reach 2^31");
        std::vector<uint32_t> pos_off(n_windows + 1, 0), prof_window, prof_pos, prof_n;
        std::vector<int64_t> win_start(n_windows), win_end(n_windows), contig_len(n_windows);
        uint32_t max_prof_n = 0;
        for (uint32_t w = 0; w < n_windows; ++w) {
            const std::string wd = "window " + std::to_string(w) + ": ";
            if (window_ref_off[w + 1] < window_ref_off[w]) return fail(h, wd + "window_ref_off not monotonic");
            if (window_start[w] >> 62 || window_contig_length[w] >> 62) return fail(h, wd + "position beyond 2^62");
            if (window_start[w] + window_len[w] > window_contig_length[w]) return fail(h, wd + "the window ends past the contig");
            if (window_ref_off[w + 1] - window_ref_off[w] < window_len[w])
                return fail(h, wd + std::to_string(window_ref_off[w + 1] - window_ref_off[w]) + " reference bases, the window needs " + std::to_string(window_len[w]));
            if (((uint64_t)pos_off[w] + window_len[w]) >> 31) return fail(h, "the windows' positions reach 2^31");
            pos_off[w + 1] = pos_off[w] + window_len[w];
            win_start[w] = (int64_t)window_start[w];
            win_end[w] = (int64_t)(window_start[w] + window_len[w]);  // min(outer_chunk_location.end + 1, target_len)
            contig_len[w] = (int64_t)window_contig_length[w];
            const uint32_t P = profile_size ? profile_size : window_len[w];
            for (uint32_t at = 0; at < window_len[w]; at += P) {
                prof_window.push_back(w);
                prof_pos.push_back(pos_off[w] + at);
                prof_n.push_back(std::min(P, window_len[w] - at));
                max_prof_n = std::max(max_prof_n, prof_n.back());
            }
            for (uint32_t s = 0; s < n_samples; ++s) {
                const uint64_t g = (uint64_t)w * n_samples + s;
                if (group_read_off[g + 1] < group_read_off[g])
                    return fail(h, wd + "sample " + std::to_string(s) + ": group_read_off not monotonic");
            }
        }
        const uint32_t n_pos = pos_off[n_windows], n_profiles = (uint32_t)prof_window.size(), n_ref = window_ref_off[n_windows];
        const uint32_t n_reads = group_read_off[n_groups];
        if ((uint64_t)max_prof_n + max_filter_size > 65535ull * ACT_THREADS) return fail(h, "a profile of more than 16 776 960 list entries");
        if (n_ref && !ref_bases) return fail(h, "null array");
        if (n_reads && (!read_pos || !read_cigar_off || !read_off)) return fail(h, "null array");
        if (n_reads && read_cigar_off[0]) return fail(h, "read_cigar_off does not start at 0");
        if (n_reads && read_off[0]) return fail(h, "read_off does not start at 0");
        for (uint32_t r = 0; r < n_reads; ++r) {
            if (read_cigar_off[r + 1] < read_cigar_off[r]) return fail(h, "read " + std::to_string(r) + ": read_cigar_off not monotonic");
            if (read_off[r + 1] < read_off[r]) return fail(h, "read " + std::to_string(r) + ": read_off not monotonic");
        }
        const uint32_t n_cigar = n_reads ? read_cigar_off[n_reads] : 0, n_bases = n_reads ? read_off[n_reads] : 0;
        if ((n_cigar && !read_cigar) || (n_bases && (!read_bases || !read_quals))) return fail(h, "null array");

        // ---- the walk over the CIGARs: each read's span inside its window, its slots, the windows the reference panics on ----
        std::vector<uint32_t> read_window(n_reads), read_span(n_reads);
        std::vector<int64_t> read_lo(n_reads), read_pmax_end(n_reads);
        std::vector<uint64_t> slot_off(n_reads + 1, 0), tab_off(n_reads + 1, 0);
        std::vector<int32_t> status(n_windows, 0);
        for (uint32_t w = 0; w < n_windows; ++w)
            for (uint32_t s = 0; s < n_samples; ++s) {
                const uint64_t g = (uint64_t)w * n_samples + s;
                int64_t pmax = INT64_MIN;
                for (uint32_t r = group_read_off[g]; r < group_read_off[g + 1]; ++r) {
                    const std::string rd = "read " + std::to_string(r) + " (window " + std::to_string(w) + ", sample " + std::to_string(s) + "): ";
                    if (read_pos[r] < 0 || read_pos[r] >> 62) return fail(h, rd + "pos is negative or beyond 2^62");
                    if (r > group_read_off[g] && read_pos[r] < read_pos[r - 1]) return fail(h, rd + "pos is smaller than the read's before it");
                    uint64_t ref_len = 0, consumed = 0, n_ins = 0;
                    bool ref_skip = false;
                    for (uint32_t c = read_cigar_off[r]; c < read_cigar_off[r + 1]; ++c) {
                        const uint32_t op = read_cigar[c] & 15u, len = read_cigar[c] >> 4;
                        if (op > 8 || !len) return fail(h, rd + "CIGAR element " + std::to_string(c - read_cigar_off[r]) + ": unknown operator or length 0");
                        if (op == 0 || op == 2 || op == 7 || op == 8) ref_len += len;
                        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) consumed += len;
                        n_ins += op == 1;
                        ref_skip |= op == 3;
                    }
                    if (!status[w] && ref_skip) status[w] = ACT_REF_SKIP;
                    if (!status[w] && consumed > read_off[r + 1] - read_off[r]) status[w] = ACT_CIGAR_OVERRUN;
                    read_window[r] = w;
                    // the positions the read can put a slot at: its reference span and the place of a trailing insertion
                    const int64_t lo = std::max(read_pos[r], win_start[w]), end = std::min<int64_t>(read_pos[r] + (int64_t)ref_len + 1, win_end[w]);
                    read_lo[r] = lo;
                    read_span[r] = end > lo ? (uint32_t)(end - lo) : 0;
                    pmax = std::max(pmax, end);
                    read_pmax_end[r] = pmax;
                    slot_off[r + 1] = slot_off[r] + (read_span[r] ? read_span[r] + n_ins : 0);
                    tab_off[r + 1] = tab_off[r] + (read_span[r] ? read_span[r] + 1 : 0);
                }
            }
        if (n_reads && (slot_off[n_reads] >> 40 || tab_off[n_reads] >> 40)) return fail(h, "the reads' pileup slots reach 2^40");

        // ---- tables -----------------------------------------------------------------------------------------------------
        const uint32_t G = ploidy + 1;
        const std::vector<double> term = activity_term_table(ploidy);
        const std::vector<float> &prob_of_qual = activity_prob_of_qual();
        std::vector<float> taps(kernel.size());
        for (size_t i = 0; i < kernel.size(); ++i) taps[i] = (float)kernel[i];  // gaussian_kernel[..] as f32
        const auto &T = genotype_table_of(h, ploidy, 2);
        const AfGenotypeTables GT = af_genotype_tables(T, ploidy);

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->activity_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs the caller wants; everything else lies in the device-only workspace --------------
        StageLayout L;
        const auto s_ws = L.in(win_start.data(), n_windows), s_we = L.in(win_end.data(), n_windows), s_cl = L.in(contig_len.data(), n_windows);
        const auto s_po = L.in(pos_off.data(), n_windows + 1), s_ro = L.in(window_ref_off, n_windows + 1);
        const auto s_rb = L.in(ref_bases, n_ref);
        const auto s_go = L.in(group_read_off, n_groups + 1);
        const auto s_st = L.in(status.data(), n_windows);
        const auto s_rw = L.in(read_window.data(), n_reads), s_sp = L.in(read_span.data(), n_reads);
        const auto s_rp = L.in(read_pos, n_reads), s_rl = L.in(read_lo.data(), n_reads), s_pm = L.in(read_pmax_end.data(), n_reads);
        const auto s_co = L.in(read_cigar_off, n_reads ? n_reads + 1 : 0), s_cg = L.in(read_cigar, n_cigar);
        const auto s_bo = L.in(read_off, n_reads ? n_reads + 1 : 0);
        const auto s_bb = L.in(read_bases, n_bases), s_bq = L.in(read_quals, n_bases);
        const auto s_so = L.in(slot_off.data(), n_reads + 1), s_to = L.in(tab_off.data(), n_reads + 1);
        const auto s_tm = L.in(term.data(), term.size());
        const auto s_pq = L.in(prob_of_qual.data(), prob_of_qual.size());
        const auto s_tp = L.in(taps.data(), taps.size());
        const auto s_pw = L.in(prof_window.data(), n_profiles), s_pp = L.in(prof_pos.data(), n_profiles), s_pn = L.in(prof_n.data(), n_profiles);
        const auto s_gco = L.in(T.first.data(), T.first.size()), s_gc = L.in(T.second.data(), T.second.size());
        const auto s_lc = L.in(GT.log10_comb.data(), GT.log10_comb.size());
        const auto s_ga = L.in(GT.gt_alleles.data(), GT.gt_alleles.size());
        const auto s_nl = L.in(GT.neg_log10_alleles.data(), GT.neg_log10_alleles.size());
        L.end_inputs();
        const size_t n_ps = (size_t)n_pos * n_samples, n_list = (size_t)n_pos + (size_t)n_profiles * max_filter_size;
        StageLayout D;  // the device-only workspace
        const auto w_sl = D.scratch<uint16_t>(n_reads ? slot_off[n_reads] : 0);
        const auto w_tb = D.scratch<uint32_t>(n_reads ? tab_off[n_reads] : 0);
        const auto w_sc = D.scratch<double>(n_reads);
        const auto w_mu = D.scratch<uint32_t>(n_pos);
        const auto w_wk = D.scratch<uint32_t>(n_pos), w_ao = D.scratch<uint32_t>((size_t)n_pos + 1), w_gn = D.scratch<uint32_t>(n_pos);
        const auto w_sd = D.scratch<int32_t>(n_pos);
        const auto w_pl = D.scratch<uint64_t>(n_pos);
        const auto w_pr = D.scratch<double>(2ull * n_pos);
        const auto w_kd = D.scratch<uint8_t>(2ull * n_pos);
        const auto w_nv = D.scratch<double>(n_pos), w_vp = D.scratch<double>(n_pos), w_ab = D.scratch<double>(2ull * n_pos);
        const auto w_it = D.scratch<uint32_t>(n_pos);
        const auto w_ml = D.scratch<int64_t>(2ull * n_pos);
        const auto w_af = D.scratch<uint8_t>(2ull * n_pos);
        // an output is on the device always: staged and handed over when the caller wants it, else in the workspace
        const auto o_rc = out_or_scratch(L, D, read_counts, n_ps), o_rd = out_or_scratch(L, D, ref_depth, n_ps), o_nd = out_or_scratch(L, D, non_ref_depth, n_ps);
        const auto o_gl = out_or_scratch(L, D, gl, n_ps * G);
        const auto o_pl = out_or_scratch(L, D, pl, n_ps * G);
        const auto o_sm = out_or_scratch(L, D, soft_clip_mean, n_pos);
        const auto o_sn = out_or_scratch(L, D, soft_clip_count, n_pos);
        const auto o_ql = out_or_scratch(L, D, qual, n_pos);
        const auto o_fl = out_or_scratch(L, D, af_flags, n_pos);
        const auto o_ap = out_or_scratch(L, D, (float *)is_active_prob, n_pos), o_pp = out_or_scratch(L, D, (float *)profile_prob, n_list);
        const auto o_pn = out_or_scratch(L, D, profile_len, n_profiles);
        if (!h->activity_scratch.reserve(h, D, "activity profile workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "activity profile staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->activity_scratch;

        ActivityParams p{};
        p.n_windows = n_windows;
        p.n_samples = n_samples;
        p.n_reads = n_reads;
        p.n_pos = n_pos;
        p.n_profiles = n_profiles;
        p.G = G;
        p.bq = min_base_quality;
        p.F = F;
        p.max_filter = max_filter_size;
        p.max_prob_propagation = (float)max_prob_propagation;
        p.log10_ploidy = std::log10((double)ploidy);
        p.ref_pseudo = ref_pseudo_count;
        p.indel_pseudo = indel_pseudo_count;
        p.win_start = W.dev_ptr(s_ws);
        p.win_end = W.dev_ptr(s_we);
        p.contig_len = W.dev_ptr(s_cl);
        p.pos_off = W.dev_ptr(s_po);
        p.ref_off = W.dev_ptr(s_ro);
        p.ref_bases = W.dev_ptr(s_rb);
        p.group_read_off = W.dev_ptr(s_go);
        p.win_status = W.dev_ptr(s_st);
        p.read_window = W.dev_ptr(s_rw);
        p.read_pos = W.dev_ptr(s_rp);
        p.read_lo = W.dev_ptr(s_rl);
        p.read_pmax_end = W.dev_ptr(s_pm);
        p.read_span = W.dev_ptr(s_sp);
        p.cigar_off = W.dev_ptr(s_co);
        p.cigar = W.dev_ptr(s_cg);
        p.read_off = W.dev_ptr(s_bo);
        p.read_bases = W.dev_ptr(s_bb);
        p.read_quals = W.dev_ptr(s_bq);
        p.slot_off = W.dev_ptr(s_so);
        p.tab_off = W.dev_ptr(s_to);
        p.term = W.dev_ptr(s_tm);
        p.prob_of_qual = W.dev_ptr(s_pq);
        p.taps = W.dev_ptr(s_tp);
        p.ws_slot = ws.ptr(w_sl);
        p.ws_tab = ws.ptr(w_tb);
        p.read_softclips = ws.ptr(w_sc);
        p.mult = ws.ptr(w_mu);
        p.prof_window = W.dev_ptr(s_pw);
        p.prof_pos = W.dev_ptr(s_pp);
        p.prof_n = W.dev_ptr(s_pn);
        p.max_prof_n = max_prof_n;
        p.read_counts = o_rc.dev_ptr(W, ws);
        p.ref_depth = o_rd.dev_ptr(W, ws);
        p.non_ref_depth = o_nd.dev_ptr(W, ws);
        p.gl = o_gl.dev_ptr(W, ws);
        p.pl = o_pl.dev_ptr(W, ws);
        p.softclip_mean = o_sm.dev_ptr(W, ws);
        p.softclip_count = o_sn.dev_ptr(W, ws);
        p.qual = o_ql.dev_ptr(W, ws);
        p.af_flags = o_fl.dev_ptr(W, ws);
        p.is_active_prob = o_ap.dev_ptr(W, ws);
        p.profile_prob = o_pp.dev_ptr(W, ws);
        p.profile_len = o_pn.dev_ptr(W, ws);

        // the allele-frequency kernel on the PLs where they lie: one event per position, all of one shape
        AfParams a{};
        a.n_samples = n_samples;
        const bool block = af_is_block_event(G, n_samples);
        a.n_wave_events = block ? 0 : n_pos;
        a.n_block_events = block ? n_pos : 0;
        uint32_t *const e_work = ws.ptr(w_wk), *const e_allele_off = ws.ptr(w_ao), *const e_count = ws.ptr(w_gn);
        int32_t *const e_span_del = ws.ptr(w_sd);
        uint64_t *const e_pl_off = ws.ptr(w_pl);
        double *const e_prior = ws.ptr(w_pr);
        uint8_t *const e_kind = ws.ptr(w_kd);
        a.work = e_work;
        a.allele_off = e_allele_off;
        a.genotype_count = e_count;
        a.span_del = e_span_del;
        a.pl_off = e_pl_off;
        a.pl = p.pl;
        a.prior = e_prior;
        a.kind = e_kind;
        a.gt_comp_off = W.dev_ptr(s_gco);
        a.gt_comp = W.dev_ptr(s_gc);
        a.gt_log10_comb = W.dev_ptr(s_lc);
        a.gt_alleles = W.dev_ptr(s_ga);
        a.neg_log10_alleles = W.dev_ptr(s_nl);
        a.stand_min_conf = stand_min_conf;
        a.log_10 = std::log(10.0);
        a.inv_log_10 = 1.0 / a.log_10;
        a.log1mexp_threshold = std::log(0.5);
        a.log10_p_no_variant = ws.ptr(w_nv);
        a.log10_p_variant_present = ws.ptr(w_vp);
        a.qual = p.qual;
        a.flags = p.af_flags;
        a.iterations = ws.ptr(w_it);
        a.log10_p_absent = ws.ptr(w_ab);
        a.mle_count = ws.ptr(w_ml);
        a.allele_flags = ws.ptr(w_af);

        const auto launch = [&] {
            return hip_ok(h, launch_activity_pileup(p, S), "activity_read_kernel / activity_site_kernel") &&
                   hip_ok(h, launch_activity_events(p, e_work, e_allele_off, e_count, e_span_del, e_pl_off, e_prior, e_kind, S), "activity_events_kernel") &&
                   hip_ok(h, n_pos ? launch_af(a, af_genotypes_per_lane(G), S) : hipSuccess, "phmm_af_kernel") &&
                   hip_ok(h, launch_activity_bandpass(p, S), "activity_bandpass_kernel");
        };
        if (!stage_round_trip(h, W, L, S, "activity profile", launch)) return PHMM_ERR_HIP;
        memcpy(window_status, status.data(), 4 * (size_t)n_windows);
        if (filter_size) *filter_size = F;
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_activity_profile", PHMM_FAIL_CODE)
}

}  // extern "C"
