// phmm_assembly_kmers (include/phmm.h): host side -- validation and staging.  Every step runs on the device
// (phmm_asm_kernels.hip); there is no CPU path here.  The checks, the staged inputs and the workspace are phmm_assembly_graph's
// too (phmm_asm_host.hpp).
#include <cstring>
#include <string>
#include <vector>

#include "phmm_asm_host.hpp"

using namespace phmm;

using namespace phmm_host;

namespace phmm {

int asm_check(phmm_handle *h, const char *who, const AsmInputs &in, const AsmOutputsGiven &given, AsmBatch &b) {
    const auto fail = [&](const std::string &msg) {
        h->err = std::string(who) + ": " + msg;
        return h->err_code = PHMM_ERR_INVALID_ARG;
    };
    const uint32_t n_regions = in.n_regions, n_k = in.n_k;
    const uint32_t *k = in.k, *region_ref_off = in.region_ref_off, *region_read_off = in.region_read_off, *read_off = in.read_off;
    // ---- arguments: everything is checked before anything is written ----------------------------------------------------
    if (n_k < 1 || n_k > PHMM_ASM_MAX_K_VALUES) return fail("n_k is " + std::to_string(n_k) + ", outside 1.." + std::to_string(PHMM_ASM_MAX_K_VALUES));
    if (!k) return fail("a required pointer is NULL (k)");
    for (uint32_t i = 0; i < n_k; ++i) {
        if (k[i] < 1 || k[i] > PHMM_ASM_MAX_K) return fail("k[" + std::to_string(i) + "] is " + std::to_string(k[i]) + ", outside 1.." + std::to_string(PHMM_ASM_MAX_K));
        if (i && k[i] <= k[i - 1]) return fail("k is not ascending at entry " + std::to_string(i));
    }
    if (in.min_base_quality > 255) return fail("min_base_quality is above 255");
    if (!in.read_first != !in.read_len) return fail("read_first and read_len are given together or not at all");
    if (!given.pair_ok) return fail(given.pair_msg);
    if (!n_regions) return PHMM_OK;
    if (!region_ref_off || !region_read_off || !given.region_arrays_ok) return fail("a required pointer is NULL (region arrays)");
    if (region_ref_off[0]) return fail("region_ref_off does not start at 0");
    if (region_read_off[0]) return fail("region_read_off does not start at 0");
    for (uint32_t g = 0; g < n_regions; ++g) {
        const auto rg = [g] { return "region " + std::to_string(g) + ": "; };   // (made only for a failure)
        if (region_ref_off[g + 1] < region_ref_off[g]) return fail(rg() + "region_ref_off decreases");
        if (region_read_off[g + 1] < region_read_off[g]) return fail(rg() + "region_read_off decreases");
        if (region_ref_off[g + 1] - region_ref_off[g] > PHMM_ASM_MAX_REF_BASES)
            return fail(rg() + "more than " + std::to_string(PHMM_ASM_MAX_REF_BASES) + " reference bases");
    }
    const uint32_t n_ref_bases = region_ref_off[n_regions], n_reads = region_read_off[n_regions];
    if (n_ref_bases && (!in.ref_bases || !given.ref_plane_ok)) return fail(std::string("a required pointer is NULL (") + given.ref_names + ")");
    uint32_t n_read_bases = 0;
    b.begin.assign(n_reads, 0);
    b.len.assign(n_reads, 0);
    b.read_region.assign(n_reads, 0);
    b.region_plane_off.assign((size_t)n_regions + 1, 0);
    b.long_sequence = false;
    if (n_reads) {
        if (!read_off) return fail("a required pointer is NULL (read_off)");
        if (read_off[0]) return fail("read_off does not start at 0");
        for (uint32_t r = 0; r < n_reads; ++r) {
            const auto rd = [r] { return "read " + std::to_string(r) + ": "; };
            if (read_off[r + 1] < read_off[r]) return fail(rd() + "read_off decreases");
            const uint32_t whole = read_off[r + 1] - read_off[r];
            const uint32_t first = in.read_first ? in.read_first[r] : 0, n = in.read_first ? in.read_len[r] : whole;
            if (first > whole || n > whole - first) return fail(rd() + "its window lies outside the read");
            if (n > PHMM_ASM_MAX_READ_BASES) return fail(rd() + "more than " + std::to_string(PHMM_ASM_MAX_READ_BASES) + " bases");
            b.begin[r] = read_off[r] + first;
            b.len[r] = n;
            b.long_sequence |= n > ASM_LDS_SLOTS / 2;
        }
        n_read_bases = read_off[n_reads];
        if (n_read_bases && (!in.read_bases || !in.read_quals || !given.read_plane_ok))
            return fail(std::string("a required pointer is NULL (") + given.read_names + ")");
    }
    if (((uint64_t)n_ref_bases + n_read_bases) * n_k > PHMM_ASM_MAX_POSITIONS)
        return fail("bases x n_k is above " + std::to_string(PHMM_ASM_MAX_POSITIONS));
    b.table_off.assign((size_t)n_regions + 1, 0);
    for (uint32_t g = 0; g < n_regions; ++g) {
        uint32_t bases = region_ref_off[g + 1] - region_ref_off[g];
        b.long_sequence |= bases > ASM_LDS_SLOTS / 2;
        for (uint32_t r = region_read_off[g]; r < region_read_off[g + 1]; ++r) {
            b.read_region[r] = g;
            bases += b.len[r];
        }
        b.table_off[g + 1] = b.table_off[g] + 2 * bases;
        b.region_plane_off[g + 1] = n_reads ? read_off[region_read_off[g + 1]] : 0;
    }
    b.n_regions = n_regions;
    b.n_reads = n_reads;
    b.n_ref_bases = n_ref_bases;
    b.n_read_bases = n_read_bases;
    b.n_slots = b.table_off[n_regions];
    return PHMM_OK;
}

AsmStaged asm_stage_inputs(StageLayout &L, const AsmInputs &in, const AsmBatch &b) {
    AsmStaged s;
    s.ro = L.in(in.region_ref_off, (size_t)b.n_regions + 1);
    s.rr = L.in(in.region_read_off, (size_t)b.n_regions + 1);
    s.po = L.in(b.region_plane_off.data(), (size_t)b.n_regions + 1);
    s.to = L.in(b.table_off.data(), (size_t)b.n_regions + 1);
    s.rb = L.in(b.begin.data(), b.n_reads);
    s.rl = L.in(b.len.data(), b.n_reads);
    s.rg = L.in(b.read_region.data(), b.n_reads);
    s.fb = L.in(in.ref_bases, b.n_ref_bases);
    s.db = L.in(in.read_bases, b.n_read_bases);
    s.dq = L.in(in.read_quals, b.n_read_bases);
    return s;
}

AsmWorkspace asm_plan_workspace(StageLayout &D, const AsmBatch &b, size_t nk) {
    const size_t n_ref_bases = b.n_ref_bases, n_read_bases = b.n_read_bases, n_regions = b.n_regions, n_reads = b.n_reads, n_slots = b.n_slots;
    AsmWorkspace w;
    w.fh = D.scratch<uint64_t>(n_ref_bases + n_regions);
    w.dh = D.scratch<uint64_t>(n_read_bases + n_reads);
    w.re = D.scratch<uint16_t>(n_read_bases);
    w.ss = D.scratch<uint32_t>(nk * n_reads);
    w.nr = D.scratch<uint32_t>(nk * n_reads);
    w.fd = D.scratch<uint8_t>(nk * n_ref_bases);
    w.dd = D.scratch<uint8_t>(nk * n_read_bases);
    w.st = D.scratch<uint32_t>(b.long_sequence ? nk * 2 * (n_ref_bases + n_read_bases) : 0);
    w.sc = D.scratch<unsigned long long>(nk * n_slots);
    w.sr = D.scratch<uint32_t>(nk * n_slots);
    w.sb = D.scratch<uint32_t>(nk * n_slots);
    w.si = D.scratch<uint32_t>(nk * n_slots);
    w.fs = D.scratch<uint32_t>(nk * n_ref_bases);
    w.ds = D.scratch<uint32_t>(nk * n_read_bases);
    return w;
}

bool asm_reserve_workspace(phmm_handle *h, const StageLayout &D) { return h->asm_scratch.reserve(h, D, "assembly k-mer workspace"); }

void asm_bind(AsmParams &p, phmm_handle *h, const AsmInputs &in, const AsmBatch &b, const AsmStaged &s, const AsmWorkspace &w) {
    const StagingBuffer &W = h->asm_staging;
    const DeviceScratch &ws = h->asm_scratch;
    p.n_regions = b.n_regions;
    p.n_reads = b.n_reads;
    p.n_k = in.n_k;
    p.min_base_quality = in.min_base_quality;
    p.n_ref_bases = b.n_ref_bases;
    p.n_read_bases = b.n_read_bases;
    for (uint32_t i = 0; i < in.n_k; ++i) {
        p.k[i] = in.k[i];
        uint64_t pw = 1;
        for (uint32_t j = 0; j < in.k[i]; ++j) pw *= ASM_HASH_BASE;
        p.base_pow[i] = pw;
    }
    const int bits = h->sw.asm_fingerprint_bits;
    p.fp_mask = bits > 0 && bits < 64 ? (1ull << bits) - 1 : ~0ull;
    p.n_slots = b.n_slots;
    p.region_ref_off = W.dev_ptr(s.ro);
    p.region_read_off = W.dev_ptr(s.rr);
    p.region_plane_off = W.dev_ptr(s.po);
    p.region_table_off = W.dev_ptr(s.to);
    p.read_begin = W.dev_ptr(s.rb);
    p.read_len = W.dev_ptr(s.rl);
    p.read_region = W.dev_ptr(s.rg);
    p.ref_bases = W.dev_ptr(s.fb);
    p.read_bases = W.dev_ptr(s.db);
    p.read_quals = W.dev_ptr(s.dq);
    p.ref_hash = ws.ptr(w.fh);
    p.read_hash = ws.ptr(w.dh);
    p.run_end = ws.ptr(w.re);
    p.read_scan_stop = ws.ptr(w.ss);
    p.read_n_runs = ws.ptr(w.nr);
    p.ref_dup = ws.ptr(w.fd);
    p.read_dup = ws.ptr(w.dd);
    p.seq_table = b.long_sequence ? ws.ptr(w.st) : nullptr;
    p.slot_claim = ws.ptr(w.sc);
    p.slot_rep = ws.ptr(w.sr);
    p.slot_bits = ws.ptr(w.sb);
    p.slot_id = ws.ptr(w.si);
    p.ref_slot = ws.ptr(w.fs);
    p.read_slot = ws.ptr(w.ds);
}

}  // namespace phmm

extern "C" int phmm_assembly_kmers(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                                   const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases,
                                   const uint8_t *read_quals, const uint32_t *read_first, const uint32_t *read_len, uint32_t n_k,
                                   const uint32_t *k, uint32_t min_base_quality, uint32_t *flags, uint32_t *n_sequences,
                                   uint32_t *n_non_unique, uint32_t *n_tracked, uint32_t *n_distinct, uint8_t *ref_kmer_flags,
                                   uint8_t *read_kmer_flags, uint32_t *ref_kmer_id, uint32_t *read_kmer_id) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
        h->err_code = PHMM_OK;
        const AsmInputs in{n_regions, region_ref_off, ref_bases, region_read_off, read_off, read_bases, read_quals, read_first, read_len, n_k, k, min_base_quality};
        const AsmOutputsGiven given{!ref_kmer_id == !read_kmer_id, "ref_kmer_id and read_kmer_id are given together or not at all",
                                    flags && n_sequences && n_non_unique && n_tracked && n_distinct, ref_kmer_flags != nullptr,
                                    "ref_bases, ref_kmer_flags", read_kmer_flags != nullptr, "read_bases, read_quals, read_kmer_flags"};
        AsmBatch b;
        if (const int rc = asm_check(h, "phmm_assembly_kmers", in, given, b)) return rc;
        if (!b.n_regions) return PHMM_OK;
        const uint32_t n_ref_bases = b.n_ref_bases, n_read_bases = b.n_read_bases;
        const bool ids = ref_kmer_id != nullptr;

        DeviceGuard dg(h->device);
        StagingBuffer &W = h->asm_staging;
        hipStream_t S = h->streams[0];
        // ---- staging: inputs, then the outputs; hashes, runs and tables lie in the device-only workspace -----------------------
        StageLayout L;
        const AsmStaged staged = asm_stage_inputs(L, in, b);
        L.end_inputs();
        const size_t nk = n_k, per = nk * n_regions;
        const auto o_fl = L.out(flags, per), o_ns = L.out(n_sequences, per), o_nu = L.out(n_non_unique, per), o_nt = L.out(n_tracked, per), o_nd = L.out(n_distinct, per);
        const auto o_ff = L.out(ref_kmer_flags, nk * n_ref_bases), o_df = L.out(read_kmer_flags, nk * n_read_bases);
        const auto o_fi = L.out(ref_kmer_id, ids ? nk * n_ref_bases : 0), o_di = L.out(read_kmer_id, ids ? nk * n_read_bases : 0);
        StageLayout D;  // the device-only workspace
        const AsmWorkspace ws = asm_plan_workspace(D, b, nk);
        if (!asm_reserve_workspace(h, D)) return PHMM_ERR_HIP;
        if (!W.reserve(h, L, "assembly k-mer staging")) return PHMM_ERR_HIP;
        h->stat_staged_bytes += L.in_bytes;

        AsmParams p{};
        asm_bind(p, h, in, b, staged, ws);
        p.flags = W.dev_ptr_or_null(o_fl);
        p.n_sequences = W.dev_ptr_or_null(o_ns);
        p.n_non_unique = W.dev_ptr_or_null(o_nu);
        p.n_tracked = W.dev_ptr_or_null(o_nt);
        p.n_distinct = W.dev_ptr_or_null(o_nd);
        p.ref_flags = W.dev_ptr_or_null(o_ff);
        p.read_flags = W.dev_ptr_or_null(o_df);
        p.ref_kmer_id = W.dev_ptr_or_null(o_fi);
        p.read_kmer_id = W.dev_ptr_or_null(o_di);
        p.want_ids = ids;   // (an empty plane's pointer is null and no kernel indexes it)

        if (!stage_round_trip(h, W, L, S, "assembly k-mers", [&] { return hip_ok(h, launch_assembly_kmers(p, S), "assembly k-mer kernels"); })) return PHMM_ERR_HIP;
        return PHMM_OK;
    PHMM_GUARD_END(h, "phmm_assembly_kmers", PHMM_FAIL_CODE)
}
