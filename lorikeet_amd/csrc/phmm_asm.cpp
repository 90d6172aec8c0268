// phmm_assembly_kmers (include/phmm.h): host side -- validation and staging.  Every step runs on the device
// (phmm_asm_kernels.hip); there is no CPU path here.
#include <cstring>
#include <string>
#include <vector>

#include "phmm_asm_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

using namespace phmm;

using namespace phmm_host;

namespace {

int fail(phmm_handle *h, const std::string &msg) {
    h->err = "phmm_assembly_kmers: " + msg;
    return h->err_code = PHMM_ERR_INVALID_ARG;
}

struct Out {  // an output array the caller gave: where it lies in the staging buffer
    void *user;
    size_t bytes;
    size_t off = 0;
};

}  // namespace

extern "C" int phmm_assembly_kmers(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                                   const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases,
                                   const uint8_t *read_quals, const uint32_t *read_first, const uint32_t *read_len, uint32_t n_k,
                                   const uint32_t *k, uint32_t min_base_quality, uint32_t *flags, uint32_t *n_sequences,
                                   uint32_t *n_non_unique, uint32_t *n_tracked, uint32_t *n_distinct, uint8_t *ref_kmer_flags,
                                   uint8_t *read_kmer_flags, uint32_t *ref_kmer_id, uint32_t *read_kmer_id) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        // ---- arguments: everything is checked before anything is written ----------------------------------------------------
        if (n_k < 1 || n_k > PHMM_ASM_MAX_K_VALUES) return fail(h, "n_k is " + std::to_string(n_k) + ", outside 1.." + std::to_string(PHMM_ASM_MAX_K_VALUES));
        if (!k) return fail(h, "a required pointer is NULL (k)");
        for (uint32_t i = 0; i < n_k; ++i) {
            if (k[i] < 1 || k[i] > PHMM_ASM_MAX_K) return fail(h, "k[" + std::to_string(i) + "] is " + std::to_string(k[i]) + ", outside 1.." + std::to_string(PHMM_ASM_MAX_K));
            if (i && k[i] <= k[i - 1]) return fail(h, "k is not ascending at entry " + std::to_string(i));
        }
        if (min_base_quality > 255) return fail(h, "min_base_quality is above 255");
        if (!read_first != !read_len) return fail(h, "read_first and read_len are given together or not at all");
        if (!ref_kmer_id != !read_kmer_id) return fail(h, "ref_kmer_id and read_kmer_id are given together or not at all");
        if (!n_regions) return PHMM_OK;
        if (!region_ref_off || !region_read_off || !flags || !n_sequences || !n_non_unique || !n_tracked || !n_distinct)
            return fail(h, "a required pointer is NULL (region arrays)");
        if (region_ref_off[0]) return fail(h, "region_ref_off does not start at 0");
        if (region_read_off[0]) return fail(h, "region_read_off does not start at 0");
        for (uint32_t g = 0; g < n_regions; ++g) {
            const auto rg = [g] { return "region " + std::to_string(g) + ": "; };   // (made only for a failure)
            if (region_ref_off[g + 1] < region_ref_off[g]) return fail(h, rg() + "region_ref_off decreases");
            if (region_read_off[g + 1] < region_read_off[g]) return fail(h, rg() + "region_read_off decreases");
            if (region_ref_off[g + 1] - region_ref_off[g] > PHMM_ASM_MAX_REF_BASES)
                return fail(h, rg() + "more than " + std::to_string(PHMM_ASM_MAX_REF_BASES) + " reference bases");
        }
        const uint32_t n_ref_bases = region_ref_off[n_regions], n_reads = region_read_off[n_regions];
        if (n_ref_bases && (!ref_bases || !ref_kmer_flags)) return fail(h, "a required pointer is NULL (ref_bases, ref_kmer_flags)");
        uint32_t n_read_bases = 0;
        std::vector<uint32_t> begin(n_reads), len(n_reads), read_region(n_reads), region_plane_off((size_t)n_regions + 1, 0);
        bool long_sequence = false;
        if (n_reads) {
            if (!read_off) return fail(h, "a required pointer is NULL (read_off)");
            if (read_off[0]) return fail(h, "read_off does not start at 0");
            for (uint32_t r = 0; r < n_reads; ++r) {
                const auto rd = [r] { return "read " + std::to_string(r) + ": "; };
                if (read_off[r + 1] < read_off[r]) return fail(h, rd() + "read_off decreases");
                const uint32_t whole = read_off[r + 1] - read_off[r];
                const uint32_t first = read_first ? read_first[r] : 0, n = read_first ? read_len[r] : whole;
                if (first > whole || n > whole - first) return fail(h, rd() + "its window lies outside the read");
                if (n > PHMM_ASM_MAX_READ_BASES) return fail(h, rd() + "more than " + std::to_string(PHMM_ASM_MAX_READ_BASES) + " bases");
                begin[r] = read_off[r] + first;
                len[r] = n;
                long_sequence |= n > ASM_LDS_SLOTS / 2;
            }
            n_read_bases = read_off[n_reads];
            if (n_read_bases && (!read_bases || !read_quals || !read_kmer_flags))
                return fail(h, "a required pointer is NULL (read_bases, read_quals, read_kmer_flags)");
        }
        if (((uint64_t)n_ref_bases + n_read_bases) * n_k > PHMM_ASM_MAX_POSITIONS)
            return fail(h, "bases x n_k is above " + std::to_string(PHMM_ASM_MAX_POSITIONS));
        std::vector<uint32_t> table_off((size_t)n_regions + 1, 0);
        for (uint32_t g = 0; g < n_regions; ++g) {
            uint32_t bases = region_ref_off[g + 1] - region_ref_off[g];
            long_sequence |= bases > ASM_LDS_SLOTS / 2;
            for (uint32_t r = region_read_off[g]; r < region_read_off[g + 1]; ++r) {
                read_region[r] = g;
                bases += len[r];
            }
            table_off[g + 1] = table_off[g] + 2 * bases;
            region_plane_off[g + 1] = n_reads ? read_off[region_read_off[g + 1]] : 0;
        }
        const uint32_t n_slots = table_off[n_regions];
        const bool ids = ref_kmer_id != nullptr;

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->asm_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs; hashes, runs and tables lie in the device-only workspace -----------------------
        StageLayout L;
        const auto s_ro = L.in(region_ref_off, (size_t)n_regions + 1), s_rr = L.in(region_read_off, (size_t)n_regions + 1);
        const auto s_po = L.in(region_plane_off.data(), (size_t)n_regions + 1), s_to = L.in(table_off.data(), (size_t)n_regions + 1);
        const auto s_rb = L.in(begin.data(), n_reads), s_rl = L.in(len.data(), n_reads), s_rg = L.in(read_region.data(), n_reads);
        const auto s_fb = L.in(ref_bases, n_ref_bases), s_db = L.in(read_bases, n_read_bases), s_dq = L.in(read_quals, n_read_bases);
        L.end_inputs();
        const size_t nk = n_k, per = 4 * nk * n_regions;
        Out outs[9] = {{flags, per}, {n_sequences, per}, {n_non_unique, per}, {n_tracked, per}, {n_distinct, per},
                       {ref_kmer_flags, nk * n_ref_bases}, {read_kmer_flags, nk * n_read_bases},
                       {ref_kmer_id, ids ? 4 * nk * n_ref_bases : 0}, {read_kmer_id, ids ? 4 * nk * n_read_bases : 0}};
        for (Out &o : outs) o.off = L.out<char>(o.bytes).off;
        StageLayout D;  // the device-only workspace
        const auto w_fh = D.scratch<uint64_t>((size_t)n_ref_bases + n_regions), w_dh = D.scratch<uint64_t>((size_t)n_read_bases + n_reads);
        const auto w_re = D.scratch<uint16_t>(n_read_bases);
        const auto w_ss = D.scratch<uint32_t>(nk * n_reads), w_nr = D.scratch<uint32_t>(nk * n_reads);
        const auto w_fd = D.scratch<uint8_t>(nk * n_ref_bases), w_dd = D.scratch<uint8_t>(nk * n_read_bases);
        const auto w_st = D.scratch<uint32_t>(long_sequence ? nk * 2 * ((size_t)n_ref_bases + n_read_bases) : 0);
        const auto w_sc = D.scratch<unsigned long long>(nk * n_slots);
        const auto w_sr = D.scratch<uint32_t>(nk * n_slots), w_sb = D.scratch<uint32_t>(nk * n_slots), w_si = D.scratch<uint32_t>(nk * n_slots);
        const auto w_fs = D.scratch<uint32_t>(nk * n_ref_bases), w_ds = D.scratch<uint32_t>(nk * n_read_bases);
        if (h->asm_scratch_cap < D.total) {
            for (int i = 0; i < kSlots; ++i) (void)hipStreamSynchronize(h->streams[i]);
            if (h->asm_scratch) (void)hipFree(h->asm_scratch);
            h->asm_scratch = nullptr;
            h->asm_scratch_cap = 0;
            const size_t bytes = D.total + D.total / 2;
            char *ws = nullptr;
            if (!hip_ok(h, hipMalloc((void **)&ws, bytes), "hipMalloc(assembly k-mer workspace)")) return PHMM_ERR_HIP;
            h->asm_scratch = ws;
            h->asm_scratch_cap = bytes;
        }
        if (!W.reserve(h, L, "assembly k-mer staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;
        char *const ws = h->asm_scratch;
        auto out_ptr = [&](int i) -> void * { return outs[i].bytes ? W.dev + outs[i].off : nullptr; };

        AsmParams p{};
        p.n_regions = n_regions;
        p.n_reads = n_reads;
        p.n_k = n_k;
        p.min_base_quality = min_base_quality;
        p.n_ref_bases = n_ref_bases;
        p.n_read_bases = n_read_bases;
        for (uint32_t i = 0; i < n_k; ++i) {
            p.k[i] = k[i];
            uint64_t pw = 1;
            for (uint32_t j = 0; j < k[i]; ++j) pw *= ASM_HASH_BASE;
            p.base_pow[i] = pw;
        }
        const int bits = h->sw.asm_fingerprint_bits;
        p.fp_mask = bits > 0 && bits < 64 ? (1ull << bits) - 1 : ~0ull;
        p.n_slots = n_slots;
        p.region_ref_off = W.dev_ptr(s_ro);
        p.region_read_off = W.dev_ptr(s_rr);
        p.region_plane_off = W.dev_ptr(s_po);
        p.region_table_off = W.dev_ptr(s_to);
        p.read_begin = W.dev_ptr(s_rb);
        p.read_len = W.dev_ptr(s_rl);
        p.read_region = W.dev_ptr(s_rg);
        p.ref_bases = W.dev_ptr(s_fb);
        p.read_bases = W.dev_ptr(s_db);
        p.read_quals = W.dev_ptr(s_dq);
        p.ref_hash = (uint64_t *)(ws + w_fh.off);
        p.read_hash = (uint64_t *)(ws + w_dh.off);
        p.run_end = (uint16_t *)(ws + w_re.off);
        p.read_scan_stop = (uint32_t *)(ws + w_ss.off);
        p.read_n_runs = (uint32_t *)(ws + w_nr.off);
        p.ref_dup = (uint8_t *)(ws + w_fd.off);
        p.read_dup = (uint8_t *)(ws + w_dd.off);
        p.seq_table = long_sequence ? (uint32_t *)(ws + w_st.off) : nullptr;
        p.slot_claim = (unsigned long long *)(ws + w_sc.off);
        p.slot_rep = (uint32_t *)(ws + w_sr.off);
        p.slot_bits = (uint32_t *)(ws + w_sb.off);
        p.slot_id = (uint32_t *)(ws + w_si.off);
        p.ref_slot = (uint32_t *)(ws + w_fs.off);
        p.read_slot = (uint32_t *)(ws + w_ds.off);
        p.flags = (uint32_t *)out_ptr(0);
        p.n_sequences = (uint32_t *)out_ptr(1);
        p.n_non_unique = (uint32_t *)out_ptr(2);
        p.n_tracked = (uint32_t *)out_ptr(3);
        p.n_distinct = (uint32_t *)out_ptr(4);
        p.ref_flags = (uint8_t *)out_ptr(5);
        p.read_flags = (uint8_t *)out_ptr(6);
        p.ref_kmer_id = (uint32_t *)out_ptr(7);
        p.read_kmer_id = (uint32_t *)out_ptr(8);
        p.want_ids = ids;   // (an empty plane's pointer is null and no kernel indexes it)

        if (!hip_ok(h, hipMemcpyAsync(W.dev, W.host, L.in_bytes, hipMemcpyHostToDevice, S), "H2D assembly k-mers") ||
            !hip_ok(h, launch_assembly_kmers(p, S), "assembly k-mer kernels") ||
            !hip_ok(h, hipMemcpyAsync(W.host + L.out_begin, W.dev + L.out_begin, L.total - L.out_begin, hipMemcpyDeviceToHost, S), "D2H assembly k-mers") ||
            !hip_ok(h, hipStreamSynchronize(S), "sync(assembly k-mers)"))
            return PHMM_ERR_HIP;
        for (const Out &o : outs)
            if (o.bytes) memcpy(o.user, W.host + o.off, o.bytes);
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_kmers", PHMM_FAIL_CODE)
}
