// phmm_assembly_regions (include/phmm.h): host side -- validation, the prefix sums that place a profile's words and slab, staging.
// Every step runs on the device (phmm_regions_kernels.hip); there is no CPU path here.  The call waits for the device twice
// before its last copy: once for the number of regions, once for the number of memberships, so that everything behind either
// is sized exactly and not for the worst case (a region per state, every read in every region).
#include <cstring>
#include <string>
#include <vector>

#include "phmm_host.hpp"
#include "phmm_regions_internal.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_regions: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int phmm_assembly_regions(phmm_handle *h, uint32_t n_profiles, uint32_t n_windows, uint32_t n_samples,
                                     uint32_t assembly_region_extension, uint32_t min_region_size, uint32_t max_region_size,
                                     uint32_t max_prob_propagation, double active_prob_threshold, uint32_t max_input_depth,
                                     uint32_t n_prob, const void *profile_prob, const uint32_t *profile_first,
                                     const uint32_t *profile_len, const uint64_t *profile_start, const uint64_t *profile_stop,
                                     const uint64_t *profile_contig_length, const uint32_t *profile_window,
                                     const uint32_t *group_read_off, const int64_t *read_pos, const uint32_t *read_cigar_off,
                                     const uint32_t *read_cigar, const uint32_t *read_off, const uint8_t *read_quals,
                                     const uint32_t *capacity, uint32_t *required, int32_t *profile_status,
                                     uint32_t *profile_region_off, uint64_t *region_start, uint64_t *region_end,
                                     uint64_t *region_padded_start, uint64_t *region_padded_end, uint32_t *region_states,
                                     uint32_t *region_flags, void *region_density, uint32_t *region_n_reads,
                                     uint32_t *region_read_off, uint32_t *region_reads, double *read_mean_qual) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!min_region_size) return fail(h, "min_region_size must be >= 1");  // the reference's assertions (:378-379)
        if (!max_region_size) return fail(h, "max_region_size must be >= 1");
        if (!capacity || !required || !profile_region_off) return fail(h, "null array (capacity, required, profile_region_off)");
        const bool reads = group_read_off != nullptr;
        if (!n_profiles) {
            required[0] = required[1] = 0;
            profile_region_off[0] = 0;
            if (reads && region_read_off) region_read_off[0] = 0;
            return PHMM_OK;
        }
        if (!profile_first || !profile_len || !profile_start || !profile_stop || !profile_contig_length || !profile_status)
            return fail(h, "null array (profile inputs, profile_status)");
        if (capacity[0] && (!region_start || !region_end || !region_padded_start || !region_padded_end || !region_states || !region_flags ||
                            !region_density || !region_n_reads))
            return fail(h, "null array (region outputs)");
        if (reads && !n_samples) return fail(h, "no samples");
        if (reads && !profile_window) return fail(h, "null array (profile_window)");
        if (reads && ((capacity[0] && !region_read_off) || (capacity[1] && !region_reads))) return fail(h, "null array (region_read_off, region_reads)");
        std::vector<uint32_t> state_off(n_profiles + 1, 0), word_off(n_profiles + 1, 0);
        for (uint32_t k = 0; k < n_profiles; ++k) {
            const auto pf = [k] { return "profile " + std::to_string(k) + ": "; };
            if ((uint64_t)profile_first[k] + profile_len[k] > n_prob) return fail(h, pf() + "profile_first + profile_len is past profile_prob");
            if (!profile_contig_length[k]) return fail(h, pf() + "contig length 0");  // trim_interval_to_contig's assertion
            if (profile_start[k] >> 62 || profile_stop[k] >> 62 || profile_contig_length[k] >> 62) return fail(h, pf() + "position beyond 2^62");
            if (reads && profile_window[k] >= n_windows) return fail(h, pf() + "window " + std::to_string(profile_window[k]) + " of " + std::to_string(n_windows));
            const uint64_t states = (uint64_t)state_off[k] + profile_len[k];
            if ((states * (reads ? n_samples : 1)) >> 31) return fail(h, "states x samples reach 2^31");
            state_off[k + 1] = (uint32_t)states;
            word_off[k + 1] = word_off[k] + (profile_len[k] + 63) / 64;
        }
        const uint32_t n_states = state_off[n_profiles], n_words = word_off[n_profiles];
        if (n_states && !profile_prob) return fail(h, "null array (profile_prob)");
        const uint64_t n_groups = reads ? (uint64_t)n_windows * n_samples : 0;
        if (n_groups >> 31) return fail(h, "windows x samples reach 2^31");
        uint32_t n_reads = 0, n_cigar = 0, n_quals = 0;
        if (reads) {
            if (group_read_off[0]) return fail(h, "group_read_off does not start at 0");
            for (uint64_t g = 0; g < n_groups; ++g)
                if (group_read_off[g + 1] < group_read_off[g]) return fail(h, "group " + std::to_string(g) + ": group_read_off not monotonic");
            n_reads = group_read_off[n_groups];
            if (n_reads && (!read_pos || !read_cigar_off || !read_off)) return fail(h, "null array (read_pos, read_cigar_off, read_off)");
            if (n_reads && read_cigar_off[0]) return fail(h, "read_cigar_off does not start at 0");
            if (n_reads && read_off[0]) return fail(h, "read_off does not start at 0");
            for (uint32_t r = 0; r < n_reads; ++r) {
                if (read_cigar_off[r + 1] < read_cigar_off[r]) return fail(h, "read " + std::to_string(r) + ": read_cigar_off not monotonic");
                if (read_off[r + 1] < read_off[r]) return fail(h, "read " + std::to_string(r) + ": read_off not monotonic");
            }
            n_cigar = n_reads ? read_cigar_off[n_reads] : 0;
            n_quals = n_reads ? read_off[n_reads] : 0;
            if ((n_cigar && !read_cigar) || (n_quals && !read_quals)) return fail(h, "null array (read_cigar, read_quals)");
            for (uint64_t g = 0; g < n_groups; ++g)
                for (uint32_t r = group_read_off[g]; r < group_read_off[g + 1]; ++r) {
                    if (read_pos[r] < 0 || read_pos[r] >> 62) return fail(h, "read " + std::to_string(r) + ": pos is negative or beyond 2^62");
                    if (r > group_read_off[g] && read_pos[r] < read_pos[r - 1])
                        return fail(h, "read " + std::to_string(r) + ": pos is smaller than the read's before it");
                }
            for (uint32_t c = 0; c < n_cigar; ++c)
                if ((read_cigar[c] & 15u) > 8) return fail(h, "CIGAR element " + std::to_string(c) + ": unknown operator");
        }

        DeviceGuard dg(h->device);
        hipStream_t S = h->streams[0];
        // ---- first buffer: the inputs, what is per state and per read, the profiles' results ------------------------------------
        StagingBuffer &A = h->regions_staging;
        StageLayout LA;
        const auto s_pr = LA.in((const float *)profile_prob, n_prob);
        const auto s_pf = LA.in(profile_first, n_profiles), s_pn = LA.in(profile_len, n_profiles);
        const auto s_ps = LA.in(profile_start, n_profiles), s_pe = LA.in(profile_stop, n_profiles), s_pc = LA.in(profile_contig_length, n_profiles);
        const auto s_pw = LA.in(profile_window, reads ? n_profiles : 0);
        const auto s_so = LA.in(state_off.data(), (size_t)n_profiles + 1), s_wo = LA.in(word_off.data(), (size_t)n_profiles + 1);
        const auto s_go = LA.in(group_read_off, reads ? (size_t)n_groups + 1 : 0);
        const auto s_rp = LA.in(read_pos, n_reads);
        const auto s_co = LA.in(read_cigar_off, n_reads ? (size_t)n_reads + 1 : 0), s_cg = LA.in(read_cigar, n_cigar);
        const auto s_bo = LA.in(read_off, n_reads ? (size_t)n_reads + 1 : 0);
        const auto s_bq = LA.in(read_quals, n_quals);
        LA.end_inputs();
        const auto w_pa = LA.scratch<uint64_t>(n_words), w_pm = LA.scratch<uint64_t>(n_words), w_pd = LA.scratch<uint64_t>(n_words);
        const auto w_sf = LA.scratch<uint32_t>(n_states), w_sl = LA.scratch<uint32_t>(n_states), w_sg = LA.scratch<uint32_t>(n_states);
        const auto w_cn = LA.scratch<uint32_t>(n_profiles);
        const auto w_re = LA.scratch<int64_t>(n_reads), w_rm = LA.scratch<int64_t>(n_reads);
        const auto o_st = LA.out(profile_status, n_profiles);
        const auto o_ro = LA.out(profile_region_off, (size_t)n_profiles + 1);
        const auto o_mq = LA.out(read_mean_qual, n_reads);  // (fetched and handed over only if the caller asked for it)
        if (!A.reserve(h, LA, "assembly regions staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += LA.in_bytes;

        RegionsParams p{};
        p.n_profiles = n_profiles;
        p.n_samples = reads ? n_samples : 1;
        p.n_reads = n_reads;
        p.n_words = n_words;
        p.n_groups = (uint32_t)n_groups;
        p.extension = assembly_region_extension;
        p.min_size = min_region_size;
        p.max_size = max_region_size;
        p.max_prop = max_prob_propagation;
        p.max_depth = max_input_depth;
        p.threshold = (float)active_prob_threshold;
        p.prob = A.dev_ptr(s_pr);
        p.first = A.dev_ptr(s_pf);
        p.len = A.dev_ptr(s_pn);
        p.start = A.dev_ptr(s_ps);
        p.stop = A.dev_ptr(s_pe);
        p.contig = A.dev_ptr(s_pc);
        p.window = reads ? A.dev_ptr(s_pw) : nullptr;
        p.state_off = A.dev_ptr(s_so);
        p.word_off = A.dev_ptr(s_wo);
        p.plane_active = A.dev_ptr(w_pa);
        p.plane_min = A.dev_ptr(w_pm);
        p.plane_dense = A.dev_ptr(w_pd);
        p.slab_first = A.dev_ptr(w_sf);
        p.slab_len = A.dev_ptr(w_sl);
        p.slab_flags = A.dev_ptr(w_sg);
        p.profile_count = A.dev_ptr(w_cn);
        p.profile_status = A.dev_ptr(o_st);
        p.profile_region_off = A.dev_ptr(o_ro);
        p.group_read_off = reads ? A.dev_ptr(s_go) : nullptr;
        p.read_pos = A.dev_ptr(s_rp);
        p.cigar_off = A.dev_ptr(s_co);
        p.cigar = A.dev_ptr(s_cg);
        p.read_off = A.dev_ptr(s_bo);
        p.quals = A.dev_ptr(s_bq);
        p.read_end = A.dev_ptr(w_re);
        p.read_pmax = A.dev_ptr(w_rm);
        p.read_mean_qual = A.dev_ptr(o_mq);

        const size_t a_begin = o_st.off, a_bytes = o_ro.off + 4 * ((size_t)n_profiles + 1) - o_st.off;  // status and offsets
        if (!stage_upload(h, A, LA, S, "assembly regions, profiles") ||
            !hip_ok(h, launch_regions_cut(p, S), "regions_class_kernel / regions_cut_kernel / regions_scan_kernel") ||
            !stage_fetch(h, A, a_begin, a_bytes, S, "assembly regions, profiles") || !stage_wait(h, S, "assembly regions, profiles"))
            return PHMM_ERR_HIP;
        const uint32_t R = A.host_ptr(o_ro)[n_profiles];  // <= n_states: every region drains a state
        const size_t n_pairs = reads ? (size_t)R * n_samples : 0;

        // ---- second buffer: what is per region and per (region, sample) ---------------------------------------------------------
        StagingBuffer &B = h->regions_out_staging;
        StageLayout LB;
        LB.end_inputs();
        const auto w_f0 = LB.scratch<uint32_t>(R), w_rk = LB.scratch<uint32_t>(R);
        const auto w_lo = LB.scratch<uint32_t>(n_pairs), w_hi = LB.scratch<uint32_t>(n_pairs), w_pc = LB.scratch<uint32_t>(n_pairs);
        const auto o_nm = LB.out<uint64_t>(1);
        const auto o_rs = LB.out(region_start, R), o_rE = LB.out(region_end, R), o_qs = LB.out(region_padded_start, R), o_qe = LB.out(region_padded_end, R);
        const auto o_ns = LB.out(region_states, R), o_fl = LB.out(region_flags, R);
        const auto o_dn = LB.out((float *)region_density, R);
        const auto o_nr = LB.out(region_n_reads, R);
        const auto o_rr = LB.out<uint32_t>(reads ? n_pairs + 1 : 0);
        if (!B.reserve(h, LB, "assembly regions staging (regions)")) return PHMM_ERR_HIP;
        p.n_regions = R;
        p.region_flags0 = B.dev_ptr(w_f0);
        p.region_profile = B.dev_ptr(w_rk);
        p.pair_lo = B.dev_ptr(w_lo);
        p.pair_hi = B.dev_ptr(w_hi);
        p.pair_count = B.dev_ptr(w_pc);
        p.n_memberships = B.dev_ptr(o_nm);
        p.region_start = B.dev_ptr(o_rs);
        p.region_end = B.dev_ptr(o_rE);
        p.region_padded_start = B.dev_ptr(o_qs);
        p.region_padded_end = B.dev_ptr(o_qe);
        p.region_states = B.dev_ptr(o_ns);
        p.region_flags = B.dev_ptr(o_fl);
        p.region_density = B.dev_ptr(o_dn);
        p.region_n_reads = B.dev_ptr(o_nr);
        p.region_read_off = B.dev_ptr(o_rr);
        if (!hip_ok(h, launch_regions_spans(p, S), "regions_span_kernel ... regions_finish_kernel") || !stage_download(h, B, LB, S, "assembly regions, regions"))
            return PHMM_ERR_HIP;
        const uint64_t M = reads && R ? *B.host_ptr(o_nm) : 0;  // (without reads or regions no kernel writes it)
        if (M >> 32) return fail(h, "the regions' reads reach 2^32 entries");
        required[0] = R;
        required[1] = (uint32_t)M;
        for (int c = 0; c < 2; ++c)
            if (required[c] > capacity[c]) {
                h->err = "phmm_assembly_regions: capacity " + std::to_string(c) + " is " + std::to_string(capacity[c]) + ", " + std::to_string(required[c]) + " needed";
                return h->err_code = PHMM_ERR_EVENT_CAPACITY;
            }
        // ---- third buffer: the memberships ------------------------------------------------------------------------------------------
        StagingBuffer &Cb = h->regions_reads_staging;
        StageLayout LC;
        LC.end_inputs();
        const auto o_rd = LC.out(region_reads, M);
        if (M) {
            if (!Cb.reserve(h, LC, "assembly regions staging (reads)")) return PHMM_ERR_HIP;
            p.region_reads = Cb.dev_ptr(o_rd);
            if (!hip_ok(h, launch_regions_members(p, S), "regions_members_kernel") || !stage_fetch(h, Cb, o_rd.off, 4 * (size_t)M, S, "assembly regions, reads"))
                return PHMM_ERR_HIP;
        }
        if (n_reads && read_mean_qual && !stage_fetch(h, A, o_mq.off, 8 * (size_t)n_reads, S, "assembly regions, read_mean_qual")) return PHMM_ERR_HIP;
        if (!stage_wait(h, S, "assembly regions")) return PHMM_ERR_HIP;

        LA.hand_over(A.host);
        LB.hand_over(B.host);
        if (reads && region_read_off) {
            if (R) memcpy(region_read_off, B.host_ptr(o_rr), 4 * (n_pairs + 1));
            else region_read_off[0] = 0;
        }
        LC.hand_over(Cb.host);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_regions", PHMM_FAIL_CODE)
}
