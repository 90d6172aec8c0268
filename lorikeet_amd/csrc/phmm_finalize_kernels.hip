// phmm_finalize_reads (include/phmm.h): what the reference does to a region's reads before it assembles and before it
// genotypes -- AssemblyBasedCallerUtils::finalize_regions up to its first sort (assembly_based_caller_utils.rs:97-172),
// AssemblyRegion::trim_with_padded_span's map + filter (assembly_region.rs:341-352), clean_overlapping_read_pairs (:263-289).
// Four kernels on one stream, each a stage the next one needs finished for every read:
//   finalize_soft_clip_kernel   a lane per read: the soft clips hard-clipped or reverted (phmm_finalize_internal.hpp)
//   finalize_tail_scan_kernel   FIN_SCAN_LANES lanes per read: the two loops of clip_low_qual_ends as ballots over the window the
//                               first stage left; the same lanes copy the read's qualities to out_quals
//   finalize_clip_kernel        a lane per read: the tails, the adaptor, the region, the filter, the outputs
//   finalize_pair_kernel        a wave per pair: the overlap's qualities, 64 bases a pass
// No atomics and no appends: every output element has one writer, so a call's bytes do not depend on the batch.
#include "phmm_finalize_internal.hpp"

namespace phmm {

namespace {

using namespace findev;

__global__ __launch_bounds__(FIN_THREADS) void finalize_soft_clip_kernel(const FinalizeParams p) {
    const uint32_t r = blockIdx.x * FIN_THREADS + threadIdx.x;
    if (r < p.n_reads) stage_soft_clips(p, r);
}

__global__ __launch_bounds__(FIN_THREADS) void finalize_tail_scan_kernel(const FinalizeParams p) {
    const uint32_t t = blockIdx.x * FIN_THREADS + threadIdx.x;
    const uint32_t r = t / FIN_SCAN_LANES, l = t % FIN_SCAN_LANES;
    if (r >= p.n_reads) return;   // (whole groups leave: n_reads is tested per group)
    const uint32_t shift = (threadIdx.x % 64u) & ~(FIN_SCAN_LANES - 1u);   // where the group's lanes lie in the wave's ballot
    const uint32_t off = p.read_off[r], total = p.read_off[r + 1] - off;
    for (uint32_t i = l; i < total; i += FIN_SCAN_LANES) p.out_quals[off + i] = p.read_quals[off + i];
    const uint8_t *q = p.read_quals + off + p.st_first[r];
    const uint32_t len = p.st_len[r], low = p.min_tail_quality;
    // read_clipper.rs:508-516: the right index stops at the last base above low_qual and never goes below 0; the left index
    // at the first such base, or at the length.  The trip counts are the same for the lanes of a group.
    uint32_t left = len, right = 0;
    for (uint32_t base = 0; base < len; base += FIN_SCAN_LANES) {
        const uint32_t i = base + l;
        const bool high = i < len && q[i] > low;
        const uint32_t bits = (uint32_t)(__ballot(high) >> shift) & 0xffffu;
        if (bits) {
            left = base + (uint32_t)__ffs(bits) - 1u;
            break;
        }
    }
    for (uint32_t end = len; end > 0;) {
        const uint32_t base = end > FIN_SCAN_LANES ? end - FIN_SCAN_LANES : 0, i = base + l;
        const bool high = i < end && q[i] > low;
        const uint32_t bits = (uint32_t)(__ballot(high) >> shift) & 0xffffu;
        if (bits) {
            right = base + 31u - (uint32_t)__clz((int)bits);
            break;
        }
        end = base;
    }
    if (l == 0) {
        p.scan_left[r] = left;
        p.scan_right[r] = right;
    }
}

__global__ __launch_bounds__(FIN_THREADS) void finalize_clip_kernel(const FinalizeParams p) {
    const uint32_t r = blockIdx.x * FIN_THREADS + threadIdx.x;
    if (r < p.n_reads) stage_clip_and_filter(p, r);
}

__global__ __launch_bounds__(FIN_THREADS) void finalize_pair_kernel(const FinalizeParams p) {
    const uint32_t t = blockIdx.x * FIN_THREADS + threadIdx.x;
    const uint32_t i = t / 64u, lane = t % 64u;
    if (i >= p.n_reads) return;
    const int32_t mate = p.mate_index[i];
    if (mate <= (int32_t)i) return;   // no mate, or the wave of the mate does the pair
    const uint32_t j = (uint32_t)mate;
    uint64_t a_at = 0, b_at = 0;
    uint32_t n = 0;
    const int32_t st = pair_plan(p, i, j, &a_at, &b_at, &n);
    if (st) {   // the reference panics inside the pair step: both reads go
        if (lane == 0) {
            p.keep[i] = p.keep[j] = 0;
            p.status[i] = p.status[j] = st;
        }
        return;
    }
    const uint8_t half = (uint8_t)p.half_of_pcr_snv_qual;
    for (uint32_t k = lane; k < n; k += 64u) {   // fragment_utils.rs:105-120
        const uint64_t fa = a_at + k, fb = b_at + k;
        if (p.read_bases[fa] == p.read_bases[fb]) {
            p.out_quals[fa] = min(p.out_quals[fa], half);
            p.out_quals[fb] = min(p.out_quals[fb], half);
        } else {
            p.out_quals[fa] = 0;
            p.out_quals[fb] = 0;
        }
    }
}

}  // namespace

hipError_t launch_finalize(const FinalizeParams &p, hipStream_t stream) {
    if (!p.n_reads) return hipSuccess;
    const auto blocks = [](uint64_t threads) { return dim3((uint32_t)((threads + FIN_THREADS - 1) / FIN_THREADS)); };
    finalize_soft_clip_kernel<<<blocks(p.n_reads), FIN_THREADS, 0, stream>>>(p);
    finalize_tail_scan_kernel<<<blocks((uint64_t)p.n_reads * FIN_SCAN_LANES), FIN_THREADS, 0, stream>>>(p);
    finalize_clip_kernel<<<blocks(p.n_reads), FIN_THREADS, 0, stream>>>(p);
    if ((p.steps & FIN_PAIRS) && p.mate_index) finalize_pair_kernel<<<blocks((uint64_t)p.n_reads * 64u), FIN_THREADS, 0, stream>>>(p);
    return hipGetLastError();
}

}  // namespace phmm
