// phmm_assembly_kmers (include/phmm.h): what the reference's read-threading assembler decides from k-mers alone, in front of the
// graph -- add_read's runs (read_threading_graph.rs:341-403), determine_non_unique_kmers (:111-187), find_start (:569-588), the
// positions thread_sequence visits (:484-561), what track_kmer enters into kmer_to_vertex_map (:635-639) and the verdicts of
// create_graph (read_threading_assembler.rs:935-956) and is_low_quality_graph (:261-263) -- for many regions and several k at
// once.  Integers and bytes only.  Five kernels on one stream, each a stage the next one needs finished everywhere:
//   asm_prepare_kernel    a wave per sequence, 64 bases a pass: the prefix hash (a wave scan, one for every k), and per read
//                         the end of each base's run from a ballot of "usable", its runs of k bases or more and the last one's stop
//   asm_sequence_kernel   a block per (sequence, k): the positions 0 ..= stop - k into the sequence's own table (LDS where it
//                         fits, the workspace where not) to find its duplicates, then into the region's table
//   asm_start_kernel      a wave per (sequence, k): per run the first position in [start, stop - k) whose k-mer is not
//                         non-unique, by ballots; what is threaded from there, OR-ed into the slots
//   asm_finish_kernel     a block per (region, k): FIRST, the ids as a prefix sum of FIRST in input order, the counts and verdicts
//   asm_id_kernel         a lane per (k, position): the id of its slot (only when ids are asked for)
// Which position claims a slot, and which slot a k-mer gets, is a race; no output shows it.  What is read of a slot afterwards
// is the set of positions that met in it (equal bytes), the lowest key among them (atomicMin) and the OR of their bits, none
// of which depends on the order of arrival.  Every output element has one writer per kernel.
#include "phmm_asm_internal.hpp"

namespace phmm {

namespace {

using namespace asm_device;

__device__ inline bool usable(const AsmParams &p, const uint8_t *bases, const uint8_t *quals, uint32_t i) {
    return (bases[i] & 0xdf) != 'N' && quals[i] >= p.min_base_quality;   // read_threading_graph.rs:400-403
}

__global__ __launch_bounds__(ASM_THREADS) void asm_prepare_kernel(AsmParams p) {
    const uint32_t lane = threadIdx.x & 63, w = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= p.n_regions + p.n_reads) return;
    const bool is_read = w >= p.n_regions;
    const uint32_t r = w - p.n_regions;
    const Seq s = is_read ? read_seq(p, r) : ref_seq(p, w);
    // hash[i + 1] = hash[i] * B + (byte + 1) modulo 2^64: the scan of a pass is sum_j c_j B^(l - j), the carry comes in times B^(l + 1)
    uint64_t pw = 1;
    {
        uint64_t b = ASM_HASH_BASE;
        for (uint32_t e = lane + 1; e; e >>= 1, b *= b)
            if (e & 1) pw *= b;
    }
    unsigned long long carry = 0;
    if (lane == 0) s.hash[0] = 0;
    for (uint32_t base = 0; base < s.len; base += 64) {
        const uint32_t pos = base + lane;
        unsigned long long a = pos < s.len ? (unsigned long long)s.bases[pos] + 1 : 0;
        uint64_t bd = ASM_HASH_BASE;
        for (uint32_t d = 1; d < 64; d <<= 1, bd *= bd) {
            const unsigned long long t = __shfl_up(a, d);
            if (lane >= d) a += t * bd;
        }
        const unsigned long long hv = carry * pw + a;
        if (pos < s.len) s.hash[pos + 1] = hv;
        carry = __shfl(hv, 63);
    }
    if (!is_read) return;
    // add_read (read_threading_graph.rs:341-390): from the last pass to the first, so that a run that crosses passes knows its end
    const uint8_t *quals = p.read_quals + s.plane;
    uint16_t *run_end = p.run_end + s.plane;
    uint32_t cnt[ASM_MAX_K_VALUES], stop[ASM_MAX_K_VALUES];
#pragma unroll
    for (uint32_t kk = 0; kk < ASM_MAX_K_VALUES; ++kk) cnt[kk] = stop[kk] = 0;
    uint32_t next_bad = s.len;
    for (int pass = (int)((s.len + 63) / 64) - 1; pass >= 0; --pass) {
        const uint32_t base = (uint32_t)pass * 64, pos = base + lane;
        const bool u = pos < s.len && usable(p, s.bases, quals, pos);
        const unsigned long long bad = ~__ballot(u), above = bad >> lane;
        const uint32_t end = above ? pos + (uint32_t)__ffsll((long long)above) - 1 : next_bad;
        if (pos < s.len) run_end[pos] = (uint16_t)end;
        const bool is_start = u && (pos == 0 || !usable(p, s.bases, quals, pos - 1));
#pragma unroll
        for (uint32_t kk = 0; kk < ASM_MAX_K_VALUES; ++kk) {
            if (kk >= p.n_k) continue;
            const unsigned long long b = __ballot(is_start && end - pos >= p.k[kk]);
            cnt[kk] += (uint32_t)__popcll(b);
            const uint32_t top_end = __shfl(end, b ? 63 - __clzll((long long)b) : 0);
            if (b && !stop[kk]) stop[kk] = top_end;
        }
        if (bad) next_bad = base + (uint32_t)__ffsll((long long)bad) - 1;
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t kk = 0; kk < ASM_MAX_K_VALUES; ++kk) {
            if (kk >= p.n_k) continue;
            p.read_n_runs[(size_t)kk * p.n_reads + r] = cnt[kk];
            p.read_scan_stop[(size_t)kk * p.n_reads + r] = stop[kk];
        }
    }
}

// determine_non_unique_kmers (read_threading_graph.rs:111-141) scans 0 ..= stop - k of a sequence: FROM 0, whatever its start.
// The scans of a read's runs are prefixes of one another, so its last run's scan holds the others'.
__global__ void asm_sequence_kernel(AsmParams p, uint32_t reads) {
    __shared__ uint32_t lds[ASM_LDS_SLOTS];
    const uint32_t kk = blockIdx.y, k = p.k[kk];
    const Seq s = reads ? read_seq(p, blockIdx.x) : ref_seq(p, blockIdx.x);
    const uint32_t g = s.region;
    if (ref_len(p, g) < k) return;
    const uint32_t stop = reads ? p.read_scan_stop[(size_t)kk * p.n_reads + blockIdx.x] : s.len;
    if (stop < k) return;
    const uint32_t n_pos = stop - k + 1, cap = 2 * n_pos;
    uint32_t *tab = lds;
    if (cap > ASM_LDS_SLOTS)
        tab = p.seq_table + (size_t)kk * 2 * ((size_t)p.n_ref_bases + p.n_read_bases) + 2 * ((size_t)(reads ? p.n_ref_bases : 0) + s.plane);
    for (uint32_t i = threadIdx.x; i < cap; i += blockDim.x) tab[i] = ASM_EMPTY;
    __syncthreads();
    const size_t plane = (size_t)kk * (reads ? p.n_read_bases : p.n_ref_bases) + s.plane;
    uint8_t *dup = (reads ? p.read_dup : p.ref_dup) + plane;
    uint32_t *slot_of = (reads ? p.read_slot : p.ref_slot) + plane;
    const uint32_t t0 = p.region_table_off[g], rcap = p.region_table_off[g + 1] - t0;
    const uint32_t tbase = kk * p.n_slots + t0;
    for (uint32_t pos = threadIdx.x; pos < n_pos; pos += blockDim.x) {
        const uint64_t fp = fingerprint(p, s.hash, pos, kk);
        bool d = false;
        for (uint32_t slot = home_slot(fp, cap);; slot = slot + 1 == cap ? 0 : slot + 1) {
            const uint32_t prev = atomicCAS(&tab[slot], ASM_EMPTY, pos);
            if (prev == ASM_EMPTY) break;
            if (fingerprint(p, s.hash, prev, kk) == fp && same_bytes(s.bases + prev, s.bases + pos, k)) {
                d = true;
                break;
            }
        }
        if (d) dup[pos] = 1;   // (the occurrence that claimed the slot stays unmarked, and which one that is, is a race: read as "any" only)
        const uint32_t key = (reads ? ASM_READ_KEY : 0u) | (s.plane + pos);
        const unsigned long long want = ((unsigned long long)(uint32_t)fp << 32) | key;
        uint32_t slot = home_slot(fp, rcap);
        for (;; slot = slot + 1 == rcap ? 0 : slot + 1) {
            const unsigned long long prev = atomicCAS(&p.slot_claim[tbase + slot], ~0ull, want);
            if (prev == ~0ull) break;
            if ((uint32_t)(prev >> 32) != (uint32_t)fp) continue;
            const uint32_t pk = (uint32_t)prev;
            const uint8_t *pb = pk & ASM_READ_KEY ? p.read_bases + (pk & ~ASM_READ_KEY) : p.ref_bases + pk;
            if (same_bytes(pb, s.bases + pos, k)) break;
        }
        atomicMin(&p.slot_rep[tbase + slot], key);
        if (d) atomicOr(&p.slot_bits[tbase + slot], ASM_NON_UNIQUE);
        slot_of[pos] = tbase + slot;
    }
}

// find_start (read_threading_graph.rs:569-588) and the positions thread_sequence visits (:484-561), a run at a time
__global__ __launch_bounds__(ASM_THREADS) void asm_start_kernel(AsmParams p) {
    const uint32_t lane = threadIdx.x & 63, w = blockIdx.x * (ASM_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= p.n_regions + p.n_reads) return;
    const uint32_t kk = blockIdx.y, k = p.k[kk];
    if (w < p.n_regions) {
        // the reference: find_start returns 0; thread_sequence returns at once if len <= 0 + k, else visits 0 ..= len - k
        const Seq s = ref_seq(p, w);
        if (s.len < k) return;
        const size_t plane = (size_t)kk * p.n_ref_bases + s.plane;
        const uint32_t f = s.len > k ? ASM_THREADED : 0;
        for (uint32_t pos = lane; pos + k <= s.len; pos += 64) {
            p.ref_flags[plane + pos] = (uint8_t)(f | (pos == 0 ? ASM_THREAD_START : 0));
            if (f) atomicOr(&p.slot_bits[p.ref_slot[plane + pos]], ASM_THREADED);
        }
        return;
    }
    const uint32_t r = w - p.n_regions;
    const Seq s = read_seq(p, r);
    if (ref_len(p, s.region) < k || p.read_scan_stop[(size_t)kk * p.n_reads + r] < k) return;
    const uint16_t *run_end = p.run_end + s.plane;
    const size_t plane = (size_t)kk * p.n_read_bases + s.plane;
    bool carry = false;   // the run that crosses into this pass has its start already
    for (uint32_t base = 0; base < s.len; base += 64) {
        const uint32_t pos = base + lane;
        const bool in = pos < s.len;
        const uint32_t e = in ? run_end[pos] : pos;
        const bool u = e > pos, fits = u && pos + k <= e;
        const uint32_t slot = fits ? p.read_slot[plane + pos] : ASM_EMPTY;
        // i in start .. stop.saturating_sub(k): the bound is EXCLUSIVE, the run's last k-mer is never a start (:573-575)
        const bool cand = fits && pos + k < e && !(p.slot_bits[slot] & ASM_NON_UNIQUE);
        const bool is_start = u && (pos == 0 || run_end[pos - 1] == pos - 1);
        const unsigned long long candm = __ballot(cand), startm = __ballot(is_start);
        const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1;   // lanes 0 ..= lane
        const unsigned long long sm = startm & upto;
        const uint32_t lo = sm ? 63 - (uint32_t)__clzll((long long)sm) : 0;        // where this lane's run starts in the pass
        const bool from_before = !sm && carry;
        const unsigned long long in_run = candm & upto & ~((1ull << lo) - 1);
        const bool has = u && (from_before || in_run);
        uint32_t f = 0;
        if (fits && has) f |= ASM_THREADED;
        if (cand && !from_before && !(in_run & ~(1ull << lane))) f |= ASM_THREAD_START;
        if (in) p.read_flags[plane + pos] = (uint8_t)f;
        if (f & ASM_THREADED) atomicOr(&p.slot_bits[slot], ASM_THREADED);
        carry = __shfl((int)has, 63) != 0;
    }
}

__global__ __launch_bounds__(ASM_THREADS) void asm_finish_kernel(AsmParams p) {
    constexpr uint32_t W = ASM_THREADS / 64;
    __shared__ uint32_t sh[W][4];
    __shared__ uint32_t n_runs;
    const uint32_t g = blockIdx.x, kk = blockIdx.y, k = p.k[kk], o = kk * p.n_regions + g;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ref0 = p.region_ref_off[g], ref_n = p.region_ref_off[g + 1] - ref0;
    if (ref_n < k) {   // read_threading_assembler.rs:935-938: a failed result; nothing else is reported
        if (threadIdx.x == 0) {
            p.flags[o] = ASM_REF_SHORT;
            p.n_sequences[o] = p.n_non_unique[o] = p.n_tracked[o] = p.n_distinct[o] = 0;
        }
        return;
    }
    if (threadIdx.x == 0) n_runs = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t r = p.region_read_off[g] + threadIdx.x; r < p.region_read_off[g + 1]; r += ASM_THREADS)
        mine += p.read_n_runs[(size_t)kk * p.n_reads + r];
    if (mine) atomicAdd(&n_runs, mine);
    const uint32_t rd0 = p.region_plane_off[g], rd_n = p.region_plane_off[g + 1] - rd0, total = ref_n + rd_n;
    uint32_t distinct = 0, non_unique = 0, tracked = 0, ref_dups = 0;
    for (uint32_t base = 0; base < total; base += ASM_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const bool in = i < total, is_ref = i < ref_n;
        const size_t idx = is_ref ? (size_t)kk * p.n_ref_bases + ref0 + i : (size_t)kk * p.n_read_bases + rd0 + (i - ref_n);
        const uint32_t key = is_ref ? ref0 + i : ASM_READ_KEY | (rd0 + (i - ref_n));
        const uint32_t slot = in ? (is_ref ? p.ref_slot : p.read_slot)[idx] : ASM_EMPTY;
        const bool scanned = slot != ASM_EMPTY;
        const bool first = scanned && p.slot_rep[slot] == key;
        const uint32_t bits = scanned ? p.slot_bits[slot] : 0;
        const unsigned long long fm = __ballot(first);
        const unsigned long long nm = __ballot(first && (bits & ASM_NON_UNIQUE));
        const unsigned long long tm = __ballot(first && (bits & ASM_THREADED) && !(bits & ASM_NON_UNIQUE));
        const unsigned long long dm = __ballot(in && is_ref && p.ref_dup[idx]);
        if (lane == 0) {
            sh[wave][0] = (uint32_t)__popcll(fm);
            sh[wave][1] = (uint32_t)__popcll(nm);
            sh[wave][2] = (uint32_t)__popcll(tm);
            sh[wave][3] = (uint32_t)__popcll(dm);
        }
        __syncthreads();
        uint32_t before = 0, sum[4] = {0, 0, 0, 0};
        for (uint32_t v = 0; v < W; ++v) {
            if (v < wave) before += sh[v][0];
            for (uint32_t c = 0; c < 4; ++c) sum[c] += sh[v][c];
        }
        // ids are dense in the order of FIRST: the reference first, then the reads in input order, positions ascending
        if (first) p.slot_id[slot] = distinct + before + (uint32_t)__popcll(fm & ((1ull << lane) - 1));
        if (scanned) {
            uint8_t *fl = (is_ref ? p.ref_flags : p.read_flags) + idx;
            *fl = (uint8_t)(*fl | (bits & ASM_NON_UNIQUE) | (first ? ASM_FIRST : 0));
        }
        distinct += sum[0];
        non_unique += sum[1];
        tracked += sum[2];
        ref_dups += sum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // read_threading_assembler.rs:940-956 and read_threading_graph.rs:261-263
        p.flags[o] = (ref_dups ? ASM_REF_NON_UNIQUE : 0) | ((uint64_t)non_unique * 4 > tracked ? ASM_LOW_COMPLEXITY : 0);
        p.n_sequences[o] = n_runs + 1;
        p.n_non_unique[o] = non_unique;
        p.n_tracked[o] = tracked;
        p.n_distinct[o] = distinct;
    }
}

__global__ __launch_bounds__(ASM_THREADS) void asm_id_kernel(AsmParams p) {
    const uint32_t kk = blockIdx.y, i = blockIdx.x * ASM_THREADS + threadIdx.x;
    if (i >= p.n_ref_bases + p.n_read_bases) return;
    const bool is_ref = i < p.n_ref_bases;
    const size_t idx = is_ref ? (size_t)kk * p.n_ref_bases + i : (size_t)kk * p.n_read_bases + (i - p.n_ref_bases);
    const uint32_t slot = (is_ref ? p.ref_slot : p.read_slot)[idx];
    if (slot != ASM_EMPTY) (is_ref ? p.ref_kmer_id : p.read_kmer_id)[idx] = p.slot_id[slot];
}

}  // namespace

hipError_t launch_assembly_kmers(const AsmParams &p, hipStream_t stream) {
    hipError_t e;
    const size_t nk = p.n_k, n_ref = (size_t)nk * p.n_ref_bases, n_read = (size_t)nk * p.n_read_bases, n_slots = (size_t)nk * p.n_slots;
    const auto fill = [&](void *dst, int v, size_t bytes) { return bytes ? hipMemsetAsync(dst, v, bytes, stream) : hipSuccess; };
    if ((e = fill(p.ref_dup, 0, n_ref)) != hipSuccess || (e = fill(p.read_dup, 0, n_read)) != hipSuccess ||
        (e = fill(p.ref_slot, 0xff, 4 * n_ref)) != hipSuccess || (e = fill(p.read_slot, 0xff, 4 * n_read)) != hipSuccess ||
        (e = fill(p.slot_claim, 0xff, 8 * n_slots)) != hipSuccess || (e = fill(p.slot_rep, 0xff, 4 * n_slots)) != hipSuccess ||
        (e = fill(p.slot_bits, 0, 4 * n_slots)) != hipSuccess || (e = fill(p.ref_flags, 0, n_ref)) != hipSuccess ||
        (e = fill(p.read_flags, 0, n_read)) != hipSuccess)
        return e;
    if (p.want_ids && ((e = fill(p.ref_kmer_id, 0xff, 4 * n_ref)) != hipSuccess || (e = fill(p.read_kmer_id, 0xff, 4 * n_read)) != hipSuccess))
        return e;
    const uint32_t n_seq = p.n_regions + p.n_reads, waves = ASM_THREADS / 64;
    const dim3 seq_waves((n_seq + waves - 1) / waves, 1), seq_waves_k((n_seq + waves - 1) / waves, p.n_k);
    hipLaunchKernelGGL(asm_prepare_kernel, seq_waves, dim3(ASM_THREADS), 0, stream, p);
    hipLaunchKernelGGL(asm_sequence_kernel, dim3(p.n_regions, p.n_k), dim3(ASM_THREADS), 0, stream, p, 0u);
    if (p.n_reads) hipLaunchKernelGGL(asm_sequence_kernel, dim3(p.n_reads, p.n_k), dim3(64), 0, stream, p, 1u);
    hipLaunchKernelGGL(asm_start_kernel, seq_waves_k, dim3(ASM_THREADS), 0, stream, p);
    hipLaunchKernelGGL(asm_finish_kernel, dim3(p.n_regions, p.n_k), dim3(ASM_THREADS), 0, stream, p);
    if (p.want_ids) {
        const uint32_t n = p.n_ref_bases + p.n_read_bases;
        if (n) hipLaunchKernelGGL(asm_id_kernel, dim3((n + ASM_THREADS - 1) / ASM_THREADS, p.n_k), dim3(ASM_THREADS), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace phmm
