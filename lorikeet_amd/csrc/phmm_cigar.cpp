// phmm_project_to_reference (include/phmm.h): host side -- validation, staging, the workspace, status.  The CIGAR algebra
// itself runs on the device (phmm_cigar_kernels.hip); there is no CPU path here.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "phmm_cigar_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const char *msg) {
    h->err = std::string("phmm_project_to_reference: ") + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int phmm_project_to_reference(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                                         const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases,
                                         const uint32_t *hap_off, const uint8_t *hap_bases, const int32_t *region_ref_hap,
                                         const uint64_t *region_reference_start, const uint32_t *hap_cigar_off,
                                         const uint32_t *hap_cigar, const uint32_t *hap_start_wrt_ref, const int32_t *best_allele,
                                         const uint64_t *sw_cigar_off, const uint32_t *sw_cigar, const uint32_t *n_sw_cigar,
                                         const int32_t *sw_offset, const uint32_t *orig_cigar_off, const uint32_t *orig_cigar,
                                         const uint64_t *out_cigar_off, uint32_t *out_cigar, uint32_t *n_out_cigar,
                                         int64_t *new_pos, int32_t *status) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        latch_slot0(h);
        h->err_code = PHMM_OK;
        if (!n_regions) return PHMM_OK;
        if (!region_read_off || !region_hap_off || !region_ref_hap || !region_reference_start) return fail(h, "null array");
        if (region_read_off[0] != 0 || region_hap_off[0] != 0) return fail(h, "offset arrays must start at 0");
        for (uint32_t g = 0; g < n_regions; ++g) {
            if (region_read_off[g + 1] < region_read_off[g] || region_hap_off[g + 1] < region_hap_off[g]) return fail(h, "offsets not monotonic");
            const uint32_t nh = region_hap_off[g + 1] - region_hap_off[g];
            if (region_read_off[g + 1] > region_read_off[g] && (region_ref_hap[g] < 0 || (uint32_t)region_ref_hap[g] >= nh))
                return fail(h, "every region with reads needs its reference haplotype (region_ref_hap inside the region)");
        }
        const uint32_t n_reads = region_read_off[n_regions], n_haps = region_hap_off[n_regions];
        if (!n_reads) return PHMM_OK;
        if (!read_off || !hap_off || !hap_cigar_off || !hap_start_wrt_ref || !best_allele || !sw_cigar_off || !n_sw_cigar || !sw_offset ||
            !orig_cigar_off || !out_cigar_off || !n_out_cigar || !new_pos || !status)
            return fail(h, "null array");
        if (read_off[0] != 0 || hap_off[0] != 0 || hap_cigar_off[0] != 0 || sw_cigar_off[0] != 0 || orig_cigar_off[0] != 0 || out_cigar_off[0] != 0)
            return fail(h, "offset arrays must start at 0");
        uint32_t max_sw = 0, max_hc = 0, max_oc = 0;
        for (uint32_t a = 0; a < n_haps; ++a) {
            if (hap_off[a + 1] < hap_off[a] || hap_cigar_off[a + 1] < hap_cigar_off[a]) return fail(h, "offsets not monotonic");
            max_hc = std::max(max_hc, hap_cigar_off[a + 1] - hap_cigar_off[a]);
        }
        for (uint32_t r = 0; r < n_reads; ++r) {
            if (read_off[r + 1] < read_off[r] || sw_cigar_off[r + 1] < sw_cigar_off[r] || orig_cigar_off[r + 1] < orig_cigar_off[r] ||
                out_cigar_off[r + 1] < out_cigar_off[r])
                return fail(h, "offsets not monotonic");
            if (n_sw_cigar[r] > sw_cigar_off[r + 1] - sw_cigar_off[r]) return fail(h, "n_sw_cigar exceeds the read's slot");
            max_sw = std::max(max_sw, n_sw_cigar[r]);
            max_oc = std::max(max_oc, orig_cigar_off[r + 1] - orig_cigar_off[r]);
        }
        const size_t rb = read_off[n_reads], hb = hap_off[n_haps], n_hc = hap_cigar_off[n_haps], n_oc = orig_cigar_off[n_reads];
        const uint64_t n_sw = sw_cigar_off[n_reads], n_out = out_cigar_off[n_reads];
        if ((rb && !read_bases) || (hb && !hap_bases) || (n_hc && !hap_cigar) || (n_sw && !sw_cigar) || (n_oc && !orig_cigar) || (n_out && !out_cigar))
            return fail(h, "null array");
        // elements a lane may hold at once: the padded haplotype cigar; the projection (at most one element per pair of
        // input elements); four per element of that in left_align_indels plus two
        const uint32_t capacity = 4 * (max_sw + max_hc + 2) + 8;
        (void)max_oc;

        DeviceGuard dg(h->device);
        phmm_handle::SwWork &SW = h->swork;
        StagingBuffer &W = SW.staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then [flags | status | n_out | new_pos | out cigar] ----------------------------------------
        StageLayout L;
        const auto s_rro = L.in(region_read_off, n_regions + 1), s_rho = L.in(region_hap_off, n_regions + 1), s_ro = L.in(read_off, n_reads + 1);
        const auto s_rb = L.in(read_bases, rb);
        const auto s_ho = L.in(hap_off, n_haps + 1);
        const auto s_hb = L.in(hap_bases, hb);
        const auto s_rrh = L.in(region_ref_hap, n_regions);
        const auto s_rs = L.in(region_reference_start, n_regions);
        const auto s_hco = L.in(hap_cigar_off, n_haps + 1), s_hc = L.in(hap_cigar, n_hc), s_hs = L.in(hap_start_wrt_ref, n_haps);
        const auto s_ba = L.in(best_allele, n_reads);
        const auto s_swo = L.in(sw_cigar_off, n_reads + 1);
        const auto s_sw = L.in(sw_cigar, n_sw), s_nsw = L.in(n_sw_cigar, n_reads);
        const auto s_so = L.in(sw_offset, n_reads);
        const auto s_oco = L.in(orig_cigar_off, n_reads + 1), s_oc = L.in(orig_cigar, n_oc);
        const auto s_oo = L.in(out_cigar_off, n_reads + 1);
        L.end_inputs();
        const auto s_fl = L.out<uint32_t>(64);  // zeroed below; travels to the device with the inputs
        const auto s_st = L.out<int32_t>(n_reads);
        const auto s_no = L.out<uint32_t>(n_reads);
        const auto s_np = L.out<int64_t>(n_reads);
        const auto s_out = L.out<uint32_t>(n_out);
        if (!W.reserve(h, L, "project staging")) return PHMM_ERR_HIP;
        memset(W.host_ptr(s_fl), 0, 256);
        const size_t ws_bytes = (size_t)n_reads * 4 * capacity * 4;  // the lanes' builders live in the Smith-Waterman slab
        if (SW.slab_bytes < ws_bytes) {
            (void)hipStreamSynchronize(S);
            if (SW.slab) (void)hipFree(SW.slab);
            SW.slab = nullptr;
            SW.slab_bytes = 0;
            if (!hip_ok(h, hipMalloc((void **)&SW.slab, ws_bytes), "hipMalloc(project workspace)")) return PHMM_ERR_HIP;
            SW.slab_bytes = ws_bytes;
        }
        ProjectParams p{};
        p.n_reads = n_reads;
        p.n_regions = n_regions;
        p.region_read_off = W.dev_ptr(s_rro);
        p.region_hap_off = W.dev_ptr(s_rho);
        p.read_off = W.dev_ptr(s_ro);
        p.read_bases = W.dev_ptr(s_rb);
        p.hap_off = W.dev_ptr(s_ho);
        p.hap_bases = W.dev_ptr(s_hb);
        p.region_ref_hap = W.dev_ptr(s_rrh);
        p.region_reference_start = W.dev_ptr(s_rs);
        p.hap_cigar_off = W.dev_ptr(s_hco);
        p.hap_cigar = W.dev_ptr(s_hc);
        p.hap_start_wrt_ref = W.dev_ptr(s_hs);
        p.best_allele = W.dev_ptr(s_ba);
        p.sw_cigar_off = W.dev_ptr(s_swo);
        p.sw_cigar = W.dev_ptr(s_sw);
        p.n_sw_cigar = W.dev_ptr(s_nsw);
        p.sw_offset = W.dev_ptr(s_so);
        p.orig_cigar_off = W.dev_ptr(s_oco);
        p.orig_cigar = W.dev_ptr(s_oc);
        p.out_cigar_off = W.dev_ptr(s_oo);
        p.out_cigar = W.dev_ptr(s_out);
        p.n_out_cigar = W.dev_ptr(s_no);
        p.new_pos = W.dev_ptr(s_np);
        p.status = W.dev_ptr(s_st);
        p.flags = W.dev_ptr(s_fl);
        p.workspace = SW.slab;
        p.capacity = capacity;
        if (!hip_ok(h, hipMemcpyAsync(W.dev, W.host, L.in_bytes + 256, hipMemcpyHostToDevice, S), "H2D project") ||
            !hip_ok(h, launch_project(p, S), "phmm_project_kernel") ||
            !hip_ok(h, hipMemcpyAsync(W.host + L.out_begin, W.dev + L.out_begin, L.total - L.out_begin, hipMemcpyDeviceToHost, S), "D2H project") ||
            !hip_ok(h, hipStreamSynchronize(S), "sync(project)"))
            return PHMM_ERR_HIP;
        memcpy(status, W.host_ptr(s_st), 4ull * n_reads);
        memcpy(n_out_cigar, W.host_ptr(s_no), 4ull * n_reads);
        memcpy(new_pos, W.host_ptr(s_np), 8ull * n_reads);
        // only what the call reports: a slot's words behind the read's elements, and the slots of reads that are not
        // realigned, stay as the caller left them (the kernel wrote nothing there: the staging holds older calls' bytes)
        for (uint32_t r = 0; r < n_reads; ++r) {
            const uint64_t n = std::min<uint64_t>(n_out_cigar[r], out_cigar_off[r + 1] - out_cigar_off[r]);
            if (status[r] == CIGAR_OK && n) memcpy(out_cigar + out_cigar_off[r], W.host_ptr(s_out) + out_cigar_off[r], 4ull * n);
        }
        if (*W.host_ptr(s_fl) & 1u) {
            h->err = "phmm_project_to_reference: a CIGAR needs more elements than its slot holds (n_out_cigar has the sizes)";
            return h->err_code = PHMM_ERR_CIGAR_CAPACITY;
        }
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_project_to_reference", PHMM_FAIL_CODE)
}
