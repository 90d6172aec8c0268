// phmm_finalize_reads (include/phmm.h): host side -- validation and staging.  Every step runs on the device
// (phmm_finalize_kernels.hip); there is no CPU path here.
#include <cstring>
#include <string>
#include <vector>

#include "phmm_finalize_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_finalize_reads: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

constexpr int64_t kPosLimit = (int64_t)1 << 62;

}  // namespace

extern "C" int phmm_finalize_reads(phmm_handle *h, const void *cfg_v, uint32_t n_groups, const uint32_t *group_read_off,
                                   const uint64_t *group_span_start, const uint64_t *group_span_end, const int64_t *read_pos,
                                   const void *read_flags_v, const uint8_t *read_mapq, const int64_t *read_mpos,
                                   const int64_t *read_isize, const uint32_t *read_cigar_off, const uint32_t *read_cigar,
                                   const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *read_quals,
                                   const int32_t *mate_index, const uint64_t *out_cigar_off, int32_t *read_status, uint8_t *keep,
                                   int64_t *new_pos, uint8_t *out_unmapped, uint32_t *clip_first, uint32_t *clip_len,
                                   uint32_t *out_cigar, uint32_t *n_out_cigar, uint32_t *unclipped_len, uint32_t *lead_soft,
                                   uint32_t *trail_soft, uint8_t *out_quals) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    const phmm_finalize_config *cfg = (const phmm_finalize_config *)cfg_v;
    const uint16_t *read_flags = (const uint16_t *)read_flags_v;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (!cfg) return fail(h, "cfg is NULL");
        if (cfg->steps & ~(uint32_t)PHMM_FIN_ALL) return fail(h, "steps holds bits outside PHMM_FIN_ALL");
        if ((cfg->steps & PHMM_FIN_PAIRS) && !mate_index) return fail(h, "PHMM_FIN_PAIRS needs mate_index, which is NULL");
        if (!n_groups) return PHMM_OK;
        if (!group_read_off || !group_span_start || !group_span_end) return fail(h, "a required pointer is NULL (group arrays)");
        if (group_read_off[0]) return fail(h, "group_read_off does not start at 0");
        for (uint32_t g = 0; g < n_groups; ++g) {
            const auto gd = [g] { return "group " + std::to_string(g) + ": "; };   // (made only for a failure)
            if (group_read_off[g + 1] < group_read_off[g]) return fail(h, gd() + "group_read_off decreases");
            if (group_span_start[g] >> 62 || group_span_end[g] >> 62) return fail(h, gd() + "span position from 2^62 on");
            if (group_span_end[g] < group_span_start[g]) return fail(h, gd() + "span_end < span_start");
        }
        const uint32_t n_reads = group_read_off[n_groups];
        if (!n_reads) return PHMM_OK;
        if (!read_status || !read_pos || !read_flags || !read_mapq || !read_mpos || !read_isize || !read_cigar_off || !read_off)
            return fail(h, "a required pointer is NULL (read arrays)");
        if (out_cigar && (!out_cigar_off || !n_out_cigar)) return fail(h, "a required pointer is NULL (out_cigar without out_cigar_off or n_out_cigar)");
        if (read_cigar_off[0]) return fail(h, "read_cigar_off does not start at 0");
        if (read_off[0]) return fail(h, "read_off does not start at 0");
        if (out_cigar_off && out_cigar_off[0]) return fail(h, "out_cigar_off does not start at 0");
        for (uint32_t r = 0; r < n_reads; ++r) {
            const auto rd = [r] { return "read " + std::to_string(r) + ": "; };
            if (read_cigar_off[r + 1] < read_cigar_off[r]) return fail(h, rd() + "read_cigar_off decreases");
            if (read_off[r + 1] < read_off[r]) return fail(h, rd() + "read_off decreases");
            if (out_cigar_off && out_cigar_off[r + 1] < out_cigar_off[r]) return fail(h, rd() + "out_cigar_off decreases");
        }
        const uint32_t n_cigar = read_cigar_off[n_reads], n_bases = read_off[n_reads];
        if ((n_cigar && !read_cigar) || (n_bases && !read_quals) || (n_bases && (cfg->steps & PHMM_FIN_PAIRS) && !read_bases))
            return fail(h, "a required pointer is NULL (read_cigar, read_quals, or read_bases with PHMM_FIN_PAIRS)");
        std::vector<uint32_t> read_group(n_reads);
        std::vector<uint64_t> own_cigar_off;
        if (!out_cigar_off) own_cigar_off.assign((size_t)n_reads + 1, 0);
        for (uint32_t g = 0; g < n_groups; ++g)
            for (uint32_t r = group_read_off[g]; r < group_read_off[g + 1]; ++r) {
                const auto rd = [r, g] { return "read " + std::to_string(r) + " (group " + std::to_string(g) + "): "; };
                read_group[r] = g;
                if (read_pos[r] < 0 || read_pos[r] >= kPosLimit) return fail(h, rd() + "pos is negative or from 2^62 on");
                if (read_mpos[r] <= -kPosLimit || read_mpos[r] >= kPosLimit) return fail(h, rd() + "mpos position from 2^62 on");
                if (read_isize[r] <= -kPosLimit || read_isize[r] >= kPosLimit) return fail(h, rd() + "isize position from 2^62 on");
                uint64_t consumed = 0;
                const uint32_t n = read_cigar_off[r + 1] - read_cigar_off[r];
                for (uint32_t c = read_cigar_off[r]; c < read_cigar_off[r + 1]; ++c) {
                    const uint32_t op = read_cigar[c] & 15u, len = read_cigar[c] >> 4;
                    if (op > 8 || !len) return fail(h, rd() + "CIGAR element " + std::to_string(c - read_cigar_off[r]) + ": operator above 8 or length 0");
                    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) consumed += len;
                }
                if (consumed != read_off[r + 1] - read_off[r])
                    return fail(h, rd() + "the CIGAR's read length " + std::to_string(consumed) + " differs from the read's " + std::to_string(read_off[r + 1] - read_off[r]) + " bases");
                if (out_cigar_off) {
                    if (out_cigar_off[r + 1] - out_cigar_off[r] < (uint64_t)n + 2)
                        return fail(h, rd() + "out_cigar_off leaves room for " + std::to_string(out_cigar_off[r + 1] - out_cigar_off[r]) + " elements, " + std::to_string(n + 2) + " are needed");
                } else {
                    own_cigar_off[r + 1] = own_cigar_off[r] + n + 2;
                }
                if (mate_index && mate_index[r] != -1) {
                    const int64_t m = mate_index[r];
                    if (m < (int64_t)group_read_off[g] || m >= (int64_t)group_read_off[g + 1]) return fail(h, rd() + "mate_index " + std::to_string(m) + " is out of its group");
                    if (m == (int64_t)r) return fail(h, rd() + "mate_index is self-referential");
                    if (mate_index[m] != (int32_t)r) return fail(h, rd() + "mate_index is not symmetric");
                }
            }
        const uint64_t *cigar_room = out_cigar_off ? out_cigar_off : own_cigar_off.data();
        const uint64_t n_out = cigar_room[n_reads];

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->finalize_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs the caller wants; everything else lies in the device-only workspace --------------
        StageLayout L;
        const auto s_go = L.in(group_read_off, (size_t)n_groups + 1);
        const auto s_ss = L.in(group_span_start, n_groups), s_se = L.in(group_span_end, n_groups);
        const auto s_rg = L.in(read_group.data(), n_reads);
        const auto s_rp = L.in(read_pos, n_reads), s_mp = L.in(read_mpos, n_reads), s_is = L.in(read_isize, n_reads);
        const auto s_fl = L.in(read_flags, n_reads);
        const auto s_mq = L.in(read_mapq, n_reads);
        const auto s_co = L.in(read_cigar_off, (size_t)n_reads + 1), s_cg = L.in(read_cigar, n_cigar);
        const auto s_bo = L.in(read_off, (size_t)n_reads + 1);
        const auto s_bb = L.in(read_bases, read_bases ? n_bases : 0), s_bq = L.in(read_quals, n_bases);
        const auto s_mi = L.in(mate_index, mate_index ? n_reads : 0);
        const auto s_oo = L.in(cigar_room, (size_t)n_reads + 1);
        L.end_inputs();
        StageLayout D;  // the device-only workspace
        const auto w_cg = D.scratch<uint32_t>(2 * ((size_t)n_cigar + (size_t)n_reads * FIN_SLOT_EXTRA));
        const auto w_ps = D.scratch<int64_t>(n_reads);
        const auto w_fi = D.scratch<uint32_t>(n_reads), w_ln = D.scratch<uint32_t>(n_reads), w_nn = D.scratch<uint32_t>(n_reads);
        const auto w_fg = D.scratch<uint32_t>(n_reads), w_sl = D.scratch<uint32_t>(n_reads), w_sr = D.scratch<uint32_t>(n_reads);
        // an output is on the device always: staged and handed over when the caller wants it, else in the workspace
        const auto o_st = out_or_scratch(L, D, read_status, n_reads);
        const auto o_kp = out_or_scratch(L, D, keep, n_reads);
        const auto o_np = out_or_scratch(L, D, new_pos, n_reads);
        const auto o_um = out_or_scratch(L, D, out_unmapped, n_reads);
        const auto o_cf = out_or_scratch(L, D, clip_first, n_reads), o_cl = out_or_scratch(L, D, clip_len, n_reads);
        const auto o_cg = out_or_scratch(L, D, out_cigar, n_out, /*by_hand=*/true);
        const auto o_nc = out_or_scratch(L, D, n_out_cigar, n_reads), o_ul = out_or_scratch(L, D, unclipped_len, n_reads);
        const auto o_ls = out_or_scratch(L, D, lead_soft, n_reads), o_ts = out_or_scratch(L, D, trail_soft, n_reads);
        const auto o_oq = out_or_scratch(L, D, out_quals, n_bases);
        if (!h->finalize_scratch.reserve(h, D, "finalize workspace")) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "finalize staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        const DeviceScratch &ws = h->finalize_scratch;

        FinalizeParams p{};
        p.n_groups = n_groups;
        p.n_reads = n_reads;
        p.steps = cfg->steps;
        p.min_tail_quality = cfg->min_tail_quality;
        p.dont_use_soft_clipped_bases = cfg->dont_use_soft_clipped_bases;
        p.half_of_pcr_snv_qual = cfg->half_of_pcr_snv_qual;
        p.group_read_off = W.dev_ptr(s_go);
        p.span_start = W.dev_ptr(s_ss);
        p.span_end = W.dev_ptr(s_se);
        p.read_group = W.dev_ptr(s_rg);
        p.read_pos = W.dev_ptr(s_rp);
        p.read_mpos = W.dev_ptr(s_mp);
        p.read_isize = W.dev_ptr(s_is);
        p.read_flags = W.dev_ptr(s_fl);
        p.read_mapq = W.dev_ptr(s_mq);
        p.cigar_off = W.dev_ptr(s_co);
        p.cigar = W.dev_ptr(s_cg);
        p.read_off = W.dev_ptr(s_bo);
        p.read_bases = W.dev_ptr(s_bb);
        p.read_quals = W.dev_ptr(s_bq);
        p.mate_index = mate_index ? W.dev_ptr(s_mi) : nullptr;
        p.out_cigar_off = W.dev_ptr(s_oo);
        p.ws_cigar = ws.ptr(w_cg);
        p.st_pos = ws.ptr(w_ps);
        p.st_first = ws.ptr(w_fi);
        p.st_len = ws.ptr(w_ln);
        p.st_n = ws.ptr(w_nn);
        p.st_flags = ws.ptr(w_fg);
        p.scan_left = ws.ptr(w_sl);
        p.scan_right = ws.ptr(w_sr);
        p.status = o_st.dev_ptr(W, ws);
        p.keep = o_kp.dev_ptr(W, ws);
        p.new_pos = o_np.dev_ptr(W, ws);
        p.out_unmapped = o_um.dev_ptr(W, ws);
        p.clip_first = o_cf.dev_ptr(W, ws);
        p.clip_len = o_cl.dev_ptr(W, ws);
        p.out_cigar = o_cg.dev_ptr(W, ws);
        p.n_out_cigar = o_nc.dev_ptr(W, ws);
        p.unclipped_len = o_ul.dev_ptr(W, ws);
        p.lead_soft = o_ls.dev_ptr(W, ws);
        p.trail_soft = o_ts.dev_ptr(W, ws);
        p.out_quals = o_oq.dev_ptr(W, ws);

        if (!stage_round_trip(h, W, L, S, "finalize", [&] { return hip_ok(h, launch_finalize(p, S), "finalize kernels"); })) return PHMM_ERR_HIP;
        // out_cigar is copied read by read up to its count: the room between the reads stays as the caller left it
        if (out_cigar) {
            const uint32_t *cg = W.host_ptr(o_cg.slot), *cnt = W.host_ptr(o_nc.slot);
            for (uint32_t r = 0; r < n_reads; ++r)
                if (cnt[r]) memcpy(out_cigar + cigar_room[r], cg + cigar_room[r], 4ull * cnt[r]);
        }
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_finalize_reads", PHMM_FAIL_CODE)
}
