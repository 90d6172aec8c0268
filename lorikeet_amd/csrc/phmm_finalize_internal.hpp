// phmm_finalize_reads on the device (phmm_finalize_kernels.hip): kernel parameters, shared with phmm_finalize.cpp, and the
// reference's ReadClipper restated for one lane per read.  A read is its CIGAR in one of two slots of the workspace (the
// result of a clip is built in the other), its position and flags, and the window [first, first + len) of the input's bases
// that clipping has left: ClippingOp only ever removes bases from the two ends, so no base and no quality is copied.
// Files that include this are compiled with -ffp-contract=off (phmm_cigar_device.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "phmm_cigar_device.hpp"

namespace phmm {

constexpr uint32_t FIN_THREADS = 256;
constexpr uint32_t FIN_SCAN_LANES = 16;      // lanes that scan one read's tails side by side
constexpr uint32_t FIN_SLOT_EXTRA = 4;       // a CIGAR slot holds the read's elements + this (a clip splits one element per end)
constexpr uint32_t FIN_SOFT_CLIPS = 1, FIN_LOW_QUAL_ENDS = 2, FIN_ADAPTOR = 4, FIN_REGION = 8, FIN_PAIRS = 16;   // PHMM_FIN_*
constexpr int32_t FIN_ST_CIGAR = -1, FIN_ST_CLIP_RANGE = -2, FIN_ST_ARITHMETIC = -3, FIN_ST_PAIR = -4, FIN_ST_WORKSPACE = -5;   // PHMM_FIN_STATUS_*
constexpr uint32_t FIN_FLAG_PAIRED = 0x1, FIN_FLAG_UNMAPPED = 0x4, FIN_FLAG_MATE_UNMAPPED = 0x8, FIN_FLAG_REVERSE = 0x10, FIN_FLAG_MATE_REVERSE = 0x20;

struct FinalizeParams {
    uint32_t n_groups, n_reads;
    uint32_t steps, min_tail_quality, dont_use_soft_clipped_bases, half_of_pcr_snv_qual;
    // per group
    const uint32_t *group_read_off;   // [n_groups + 1]
    const uint64_t *span_start, *span_end;
    // per read
    const uint32_t *read_group;       // [n_reads] host-made
    const int64_t *read_pos, *read_mpos, *read_isize;
    const uint16_t *read_flags;
    const uint8_t *read_mapq;
    const uint32_t *cigar_off;        // [n_reads + 1]
    const uint32_t *cigar;
    const uint32_t *read_off;         // [n_reads + 1]
    const uint8_t *read_bases, *read_quals;
    const int32_t *mate_index;        // or nullptr
    const uint64_t *out_cigar_off;    // [n_reads + 1]
    // workspace: what the soft-clip step leaves of each read, and the two tail indices
    uint32_t *ws_cigar;               // read r: two slots of cigar_off[r + 1] - cigar_off[r] + FIN_SLOT_EXTRA elements from 2 (cigar_off[r] + r FIN_SLOT_EXTRA)
    int64_t *st_pos;
    uint32_t *st_first, *st_len, *st_n, *st_flags;   // st_flags: the BAM flags | mapq << 16 | slot << 24 | emptied << 25
    uint32_t *scan_left, *scan_right;
    // results
    int32_t *status;
    uint8_t *keep, *out_unmapped;
    int64_t *new_pos;
    uint32_t *clip_first, *clip_len, *out_cigar, *n_out_cigar, *unclipped_len, *lead_soft, *trail_soft;
    uint8_t *out_quals;
};

hipError_t launch_finalize(const FinalizeParams &p, hipStream_t stream);

namespace findev {

using namespace cigdev;

struct Read {
    uint32_t *cig, *alt;      // the CIGAR and the slot the next one is built in
    uint32_t n, cap;
    int64_t pos, mpos, isize;
    uint32_t flags, mapq;
    uint32_t first, len;
    bool emptied;
    int32_t status;           // 0, or FIN_ST_*: every step returns at once when it is set

    __device__ bool is_empty() const { return len == 0; }
    __device__ bool unmapped() const { return flags & FIN_FLAG_UNMAPPED; }
    __device__ bool reverse() const { return flags & FIN_FLAG_REVERSE; }
    __device__ int64_t get_start() const { return pos; }   // bird_tool_reads.rs:239-241
    __device__ int64_t reference_length() const {
        int64_t l = 0;
        for (uint32_t i = 0; i < n; ++i) l += ref_len_of(cig[i]);
        return l;
    }
    __device__ int64_t get_end() const {   // :243-249: checked_sub(1).unwrap_or(0)
        const int64_t l = reference_length();
        return pos + (l > 0 ? l - 1 : 0);
    }
    __device__ int64_t soft_start_i64() const {   // :91-104
        int64_t start = pos;
        for (uint32_t i = 0; i < n; ++i) {
            const int op = op_of(cig[i]);
            if (op == OP_S) start -= len_of(cig[i]);
            else if (op != OP_H) break;
        }
        return start;
    }
    __device__ int64_t soft_start() {   // :76-89, unwrapped
        const int64_t s = soft_start_i64();
        if (s < 0) status = FIN_ST_ARITHMETIC;
        return s;
    }
    __device__ uint64_t seq_len_from_cigar() const {
        uint64_t l = 0;
        for (uint32_t i = 0; i < n; ++i) l += read_len_of(cig[i]);
        return l;
    }
    __device__ void swap_slots() {
        uint32_t *t = cig;
        cig = alt;
        alt = t;
    }
};

__device__ __forceinline__ void empty_read(Read &r) {   // read_utils.rs:190-211
    r.flags |= FIN_FLAG_MATE_UNMAPPED | FIN_FLAG_UNMAPPED;
    r.mapq = 0;
    r.n = 0;
    r.len = 0;
    r.emptied = true;
}

__device__ __forceinline__ bool fin_add(Read &r, Builder &b, int op, uint32_t len) {   // .add(..).unwrap()
    const int st = b.add(elem(op, len));
    if (st == CIGAR_OK) return true;
    r.status = st == CIGAR_ERR_WORKSPACE ? FIN_ST_WORKSPACE : FIN_ST_CIGAR;
    return false;
}
__device__ __forceinline__ bool fin_make(Read &r, Builder &b) {   // .make(false).unwrap(): the result becomes the read's CIGAR
    const int st = b.make();
    if (st != CIGAR_OK) {
        r.status = st == CIGAR_ERR_WORKSPACE ? FIN_ST_WORKSPACE : FIN_ST_CIGAR;
        return false;
    }
    r.swap_slots();
    r.n = b.n;
    return true;
}

// CigarUtils::clip_cigar (cigar_utils.rs:149-256) of r's CIGAR into its other slot, which becomes the CIGAR
__device__ bool clip_cigar(Read &r, uint32_t start, uint32_t stop, int clip_op) {
    const bool clip_left = start == 0;
    Builder b;
    b.init(r.alt, r.cap, true);
    uint32_t element_start = 0;
    for (uint32_t i = 0; i < r.n; ++i) {
        const int op = op_of(r.cig[i]);
        const uint32_t len = len_of(r.cig[i]);
        if (op == OP_H) {
            if (!fin_add(r, b, OP_H, len)) return false;
            continue;
        }
        const uint32_t element_end = element_start + (on_read(op) ? len : 0);
        if (element_end <= start || element_start >= stop) {
            // edge case: deletions at edge of clipping are meaningless and we skip them
            if (on_read(op) || (element_start != start && element_start != stop))
                if (!fin_add(r, b, op, len)) return false;
        } else {
            const int64_t unclipped = clip_left ? (int64_t)element_end - stop : (int64_t)start - element_start;
            if (unclipped <= 0) {   // checked_sub is None, or 0: totally clipped
                if (on_read(op) && !fin_add(r, b, clip_op, len)) return false;
            } else {
                if ((int64_t)len < unclipped) {   // len.checked_sub(unclipped_length).unwrap()
                    r.status = FIN_ST_ARITHMETIC;
                    return false;
                }
                const uint32_t clipped = len - (uint32_t)unclipped;
                if (clip_left) {
                    if (!fin_add(r, b, clip_op, clipped) || !fin_add(r, b, op, (uint32_t)unclipped)) return false;
                } else {
                    if (!fin_add(r, b, op, (uint32_t)unclipped) || !fin_add(r, b, clip_op, clipped)) return false;
                }
            }
        }
        element_start = element_end;
    }
    return fin_make(r, b);
}

// CigarUtils::alignment_start_shift (:281-328)
__device__ int64_t alignment_start_shift(const uint32_t *cig, uint32_t n, int64_t num_clipped) {
    int64_t ref_bases_clipped = 0, element_start = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const int op = op_of(cig[i]);
        const int64_t len = len_of(cig[i]);
        if (op == OP_H) continue;
        const int64_t element_end = element_start + (on_read(op) ? len : 0);
        if (element_end <= num_clipped) {
            ref_bases_clipped += on_ref(op) ? len : 0;
        } else if (element_start < num_clipped) {
            ref_bases_clipped += on_ref(op) ? num_clipped - element_start : 0;
            break;
        }
        element_start = element_end;
    }
    return ref_bases_clipped;
}

// ReadUtils::get_read_index_for_reference_coordinate (read_utils.rs:103-148): false = (None, None)
__device__ bool read_index_for_reference_coordinate(int64_t alignment_start, const uint32_t *cig, uint32_t n, int64_t ref_coord,
                                                    int64_t *index, int *oper) {
    if (ref_coord < alignment_start) return false;
    int64_t last_read = 0, last_ref = alignment_start;
    for (uint32_t i = 0; i < n; ++i) {
        const int op = op_of(cig[i]);
        const int64_t len = len_of(cig[i]);
        const int64_t first_read = last_read, first_ref = last_ref;
        last_read += on_read(op) ? len : 0;
        last_ref += (on_ref(op) || op == OP_S) ? len : 0;
        if (first_ref <= ref_coord && ref_coord < last_ref) {
            *index = first_read + (on_read(op) ? ref_coord - first_ref : 0);
            *oper = op;
            return true;
        }
    }
    return false;
}

// ClippingOp::apply_hard_clip_bases (clipping_op.rs:201-235)
__device__ void apply_hard_clip_bases(Read &r, int64_t start, int64_t stop) {
    if (stop < start || (int64_t)r.len < stop - start + 1) {   // read.len() - (stop - start + 1)
        r.status = FIN_ST_ARITHMETIC;
        return;
    }
    const uint32_t new_length = r.len - (uint32_t)(stop - start + 1);
    if (new_length == 0) {
        empty_read(r);
        return;
    }
    const uint32_t copy_start = start == 0 ? (uint32_t)stop + 1 : 0;
    if (r.unmapped()) {   // CigarString(vec![Cigar::Match(0)])
        r.alt[0] = elem(OP_M, 0);
        r.swap_slots();
        r.n = 1;
    } else {
        const uint32_t old_n = r.n;
        if (!clip_cigar(r, (uint32_t)start, (uint32_t)stop + 1, OP_H)) return;
        if (start == 0) r.pos += alignment_start_shift(r.alt, old_n, stop + 1);   // (r.alt: the CIGAR before the clip)
    }
    r.first += copy_start;
    r.len = new_length;
}

// ClippingOp::apply_revert_soft_clipped_bases (:100-139)
__device__ void apply_revert_soft_clipped_bases(Read &r) {
    if (!r.n || !(clipping(op_of(r.cig[0])) || clipping(op_of(r.cig[r.n - 1])))) return;
    const int64_t new_start = r.soft_start_i64();
    Builder b;   // CigarUtils::revert_soft_clips (cigar_utils.rs:262-276)
    b.init(r.alt, r.cap, true);
    for (uint32_t i = 0; i < r.n; ++i) {
        const int op = op_of(r.cig[i]);
        if (!fin_add(r, b, op == OP_S ? OP_M : op, len_of(r.cig[i]))) return;
    }
    if (!fin_make(r, b)) return;
    if (new_start <= 0) {
        // the start of the unclipped read lies before the contig: the bases up to it go, and the read lands on 0
        r.pos = 0;
        apply_hard_clip_bases(r, 0, -new_start);
        if (r.status) return;
        if (!r.unmapped()) r.pos = 0;
    } else {
        r.pos = new_start;
    }
}

// ReadClipper::clip_read (read_clipper.rs:363-388) with up to two operations; start < 0 = no operation
enum : int { ALG_HARD, ALG_REVERT };
__device__ void clip_read(Read &r, int64_t start0, int64_t stop0, int64_t start1, int64_t stop1, int algorithm) {
    if (start0 < 0 && start1 < 0) return;
    for (int k = 0; k < 2; ++k) {
        const int64_t start = k ? start1 : start0;
        int64_t stop = k ? stop1 : stop0;
        if (start < 0) continue;
        const int64_t read_length = r.len;
        if (start < read_length) {   // can the clipped read still be clipped in the range requested
            if (stop >= read_length) stop = read_length - 1;
            if (algorithm == ALG_HARD) apply_hard_clip_bases(r, start, stop);
            else apply_revert_soft_clipped_bases(r);
            if (r.status) return;
        }
    }
    if (r.is_empty()) empty_read(r);
}

// ReadClipper::hard_clip_soft_clipped_bases (:395-435)
__device__ void hard_clip_soft_clipped_bases(Read &r) {
    if (r.is_empty()) return;
    int64_t read_index = 0, cut_left = -1, cut_right = -1;
    bool right_tail = false;
    for (uint32_t i = 0; i < r.n; ++i) {
        const int op = op_of(r.cig[i]);
        if (op == OP_S) {
            if (right_tail) cut_right = read_index;
            else cut_left = read_index + len_of(r.cig[i]) - 1;
        } else if (op != OP_H) {
            right_tail = true;
        }
        if (on_read(op)) read_index += len_of(r.cig[i]);
    }
    // the end is cut first, otherwise the read coordinates change
    clip_read(r, cut_right >= 0 ? cut_right : -1, r.len, cut_left >= 0 ? 0 : -1, cut_left, ALG_HARD);
}

// ReadClipper::revert_soft_clipped_bases (:441-449)
__device__ void revert_soft_clipped_bases(Read &r) {
    if (r.is_empty()) return;
    clip_read(r, 0, 0, -1, -1, ALG_REVERT);
}

// ReadClipper::clip_low_qual_ends, HardclipBases (:492-532) behind its two loops: left = the first index of the window whose
// quality is above low_qual (the length when there is none), right = the last such index above 0, else 0
__device__ void hard_clip_low_qual_ends(Read &r, uint32_t left_clip_index, uint32_t right_clip_index) {
    if (r.is_empty()) return;
    const int64_t read_length = r.len;
    if (left_clip_index > right_clip_index) {   // the entire read should be clipped
        empty_read(r);
        return;
    }
    const bool right = right_clip_index < read_length - 1, left = left_clip_index > 0;
    clip_read(r, right ? (int64_t)right_clip_index + 1 : -1, read_length - 1, left ? 0 : -1, (int64_t)left_clip_index - 1, ALG_HARD);
}

// ReadClipper::clip_by_reference_coordinates, HardclipBases (:114-210); a coordinate < 0 = None
__device__ void clip_by_reference_coordinates(Read &r, int64_t ref_start, int64_t ref_stop) {
    if (r.is_empty()) return;
    int64_t start = -1, stop = -1, index = 0;
    int op = 0;
    const int64_t soft_start = r.soft_start();   // get_soft_start().unwrap()
    if (r.status) return;
    if (ref_start < 0) {
        start = 0;
        // a stop inside a deletion gives the position behind it; the stop is inclusive, so it steps back and the deletion stays
        if (read_index_for_reference_coordinate(soft_start, r.cig, r.n, ref_stop, &index, &op)) stop = index - (on_read(op) ? 0 : 1);   // checked_sub
    } else {
        if (read_index_for_reference_coordinate(soft_start, r.cig, r.n, ref_start, &index, &op)) start = index;
        stop = (int64_t)r.len - 1;
    }
    if (start < 0 || stop < 0) return;
    if (stop > (int64_t)r.len - 1 ||                 // "Trying to clip after the end of a read"
        stop < start ||                              // "Start > Stop, this should never happen"
        (start > 0 && stop < (int64_t)r.len - 1)) {  // "Trying to clip the middle of a read"
        r.status = FIN_ST_CLIP_RANGE;
        return;
    }
    clip_read(r, start, stop, -1, -1, ALG_HARD);
}

// ReadClipper::hard_clip_both_ends_by_reference_coordinates (:234-258)
__device__ void hard_clip_both_ends_by_reference_coordinates(Read &r, int64_t left, int64_t right) {
    if (r.is_empty() || left == right) {
        empty_read(r);
        return;
    }
    clip_by_reference_coordinates(r, right, -1);
    if (r.status) return;
    // the hard clipping of adjacent deletions may have taken the left cut out of the read
    if (left > r.get_end()) empty_read(r);
    else clip_by_reference_coordinates(r, -1, left);
}

// ReadClipper::hard_clip_to_region (:63-100)
__device__ void hard_clip_to_region(Read &r, int64_t ref_start, int64_t ref_stop) {
    const int64_t start = r.get_start(), stop = r.get_end();
    const int64_t left = ref_start > 0 ? ref_start - 1 : 0;   // saturating_sub(1)
    if (start <= ref_stop && stop >= ref_start) {
        if (start < ref_start && stop > ref_stop) hard_clip_both_ends_by_reference_coordinates(r, left, ref_stop + 1);
        else if (start < ref_start) clip_by_reference_coordinates(r, -1, left);
        else if (stop > ref_stop) clip_by_reference_coordinates(r, ref_stop + 1, -1);
    } else {
        empty_read(r);
    }
}

// ReadUtils::has_well_defined_fragment_size (read_utils.rs:288-316)
__device__ bool has_well_defined_fragment_size(const Read &r) {
    if (r.isize == 0 || !(r.flags & FIN_FLAG_PAIRED) || (r.flags & (FIN_FLAG_UNMAPPED | FIN_FLAG_MATE_UNMAPPED)) ||
        r.reverse() == (bool)(r.flags & FIN_FLAG_MATE_REVERSE))
        return false;
    if (r.reverse()) return r.get_end() > r.mpos;   // the read runs right to left
    return r.get_start() <= r.mpos + r.isize;
}

// ReadClipper::hard_clip_adaptor_sequence (read_clipper.rs:458-472) over ReadUtils::get_adaptor_boundary (read_utils.rs:344-353)
// and is_inside_read (:362-364)
__device__ void hard_clip_adaptor_sequence(Read &r) {
    if (!has_well_defined_fragment_size(r)) return;   // CANNOT_COMPUTE_ADAPTOR_BOUNDARY
    uint64_t boundary;
    if (r.reverse()) {
        if (r.mpos == 0) {   // mpos as usize - 1
            r.status = FIN_ST_ARITHMETIC;
            return;
        }
        boundary = (uint64_t)r.mpos - 1;   // (a negative mpos is a huge usize: outside every read)
    } else {
        boundary = (uint64_t)r.get_start() + (uint64_t)(r.isize < 0 ? -r.isize : r.isize);
    }
    if (boundary == 0 /* CANNOT_COMPUTE_ADAPTOR_BOUNDARY */ || boundary >> 63 || (int64_t)boundary < r.get_start() || (int64_t)boundary > r.get_end()) return;
    if (r.reverse()) clip_by_reference_coordinates(r, -1, (int64_t)boundary);
    else clip_by_reference_coordinates(r, (int64_t)boundary, -1);
}

// Locatable::overlaps (simple_interval.rs:298-307) of the read with the span
__device__ bool overlaps(int64_t start, int64_t end, int64_t span_start, int64_t span_end) {
    return (span_start >= start && span_start <= end) || (span_end >= start && span_end <= end) || (start >= span_start && end <= span_end);
}

// ---- the stages of the call, one lane per read ------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t *slot_of(const FinalizeParams &p, uint32_t r, uint32_t *cap) {
    *cap = p.cigar_off[r + 1] - p.cigar_off[r] + FIN_SLOT_EXTRA;
    return p.ws_cigar + 2 * ((size_t)p.cigar_off[r] + (size_t)r * FIN_SLOT_EXTRA);
}
__device__ __forceinline__ void save_read(const FinalizeParams &p, uint32_t r, const Read &rd, const uint32_t *slot0) {
    p.st_pos[r] = rd.pos;
    p.st_first[r] = rd.first;
    p.st_len[r] = rd.len;
    p.st_n[r] = rd.n;
    p.st_flags[r] = (rd.flags & 0xffffu) | (rd.mapq << 16) | (rd.cig == slot0 ? 0u : 1u << 24) | (rd.emptied ? 1u << 25 : 0u);
    p.status[r] = rd.status;
}
__device__ __forceinline__ void load_read(const FinalizeParams &p, uint32_t r, Read &rd) {
    uint32_t *slot0 = slot_of(p, r, &rd.cap);
    const uint32_t f = p.st_flags[r];
    const bool second = (f >> 24) & 1u;
    rd.cig = slot0 + (second ? rd.cap : 0);
    rd.alt = slot0 + (second ? 0 : rd.cap);
    rd.n = p.st_n[r];
    rd.pos = p.st_pos[r];
    rd.mpos = p.read_mpos[r];
    rd.isize = p.read_isize[r];
    rd.flags = f & 0xffffu;
    rd.mapq = (f >> 16) & 0xffu;
    rd.first = p.st_first[r];
    rd.len = p.st_len[r];
    rd.emptied = (f >> 25) & 1u;
    rd.status = p.status[r];
}

// stage 1: the read as the caller gave it, and the soft-clip step (assembly_based_caller_utils.rs:124-131)
__device__ void stage_soft_clips(const FinalizeParams &p, uint32_t r) {
    Read rd;
    uint32_t *slot0 = slot_of(p, r, &rd.cap);
    rd.cig = slot0;
    rd.alt = slot0 + rd.cap;
    rd.n = p.cigar_off[r + 1] - p.cigar_off[r];
    for (uint32_t i = 0; i < rd.n; ++i) rd.cig[i] = p.cigar[p.cigar_off[r] + i];
    rd.pos = p.read_pos[r];
    rd.mpos = p.read_mpos[r];
    rd.isize = p.read_isize[r];
    rd.flags = p.read_flags[r];
    rd.mapq = p.read_mapq[r];
    rd.first = 0;
    rd.len = p.read_off[r + 1] - p.read_off[r];
    rd.emptied = false;
    rd.status = 0;
    if (p.steps & FIN_SOFT_CLIPS) {
        if (p.dont_use_soft_clipped_bases || !has_well_defined_fragment_size(rd)) hard_clip_soft_clipped_bases(rd);
        else revert_soft_clipped_bases(rd);
    }
    save_read(p, r, rd, slot0);
}

// stage 3: the low-quality tails the scan found, the adaptor, the region, the filter (:133-171; assembly_region.rs:341-352)
__device__ void stage_clip_and_filter(const FinalizeParams &p, uint32_t r) {
    Read rd;
    load_read(p, r, rd);
    uint32_t cap;
    const uint32_t *slot0 = slot_of(p, r, &cap);
    bool keep = false;
    if (!rd.status) {
        const uint32_t g = p.read_group[r];
        const int64_t span_start = (int64_t)p.span_start[g], span_end = (int64_t)p.span_end[g];
        if (p.steps & FIN_LOW_QUAL_ENDS) hard_clip_low_qual_ends(rd, p.scan_left[r], p.scan_right[r]);
        if (!rd.status && rd.get_start() <= rd.get_end()) {
            if ((p.steps & FIN_ADAPTOR) && !rd.unmapped()) hard_clip_adaptor_sequence(rd);
            if (!rd.status && !rd.is_empty() && rd.seq_len_from_cigar() > 0) {
                if (p.steps & FIN_REGION) hard_clip_to_region(rd, span_start, span_end);
                keep = !rd.status && rd.get_start() <= rd.get_end() && rd.len > 0 && overlaps(rd.get_start(), rd.get_end(), span_start, span_end);
            }
        }
    }
    uint32_t *out = p.out_cigar + p.out_cigar_off[r];
    const uint64_t out_cap = p.out_cigar_off[r + 1] - p.out_cigar_off[r];
    if (!rd.status && rd.n > out_cap) rd.status = FIN_ST_WORKSPACE;
    const bool ok = !rd.status;
    uint32_t lead = 0, trail = 0, soft = 0, not_hard = 0;
    if (ok) {
        for (uint32_t i = 0; i < rd.n; ++i) {
            out[i] = rd.cig[i];
            if (op_of(rd.cig[i]) == OP_S) soft += len_of(rd.cig[i]);
            not_hard += op_of(rd.cig[i]) != OP_H;
        }
        // the leading and the trailing soft clip behind the hard clips; a CIGAR that is one soft clip has the leading one alone
        for (uint32_t i = 0; i < rd.n; ++i) {
            if (op_of(rd.cig[i]) == OP_S) lead = len_of(rd.cig[i]);
            if (op_of(rd.cig[i]) != OP_H) break;
        }
        for (uint32_t i = rd.n; i-- > 0;) {
            if (op_of(rd.cig[i]) == OP_S) trail = len_of(rd.cig[i]);
            if (op_of(rd.cig[i]) != OP_H) break;
        }
        if (not_hard == 1 && lead) trail = 0;
    }
    save_read(p, r, rd, slot0);
    p.keep[r] = ok && keep;
    p.new_pos[r] = ok ? rd.pos : 0;
    p.out_unmapped[r] = ok && rd.emptied;
    p.clip_first[r] = ok && rd.len ? rd.first : 0;
    p.clip_len[r] = ok ? rd.len : 0;
    p.n_out_cigar[r] = ok ? rd.n : 0;
    p.unclipped_len[r] = ok ? rd.len - soft : 0;
    p.lead_soft[r] = lead;
    p.trail_soft[r] = trail;
}

// stage 4, what every lane of a pair's wave works out alike: whether reads i < j are a pair FragmentCollection::create
// (fragment_collection.rs:32-76) forms, and adjust_quals_of_overlapping_paired_fragments (fragment_utils.rs:27-149) up to its
// loop: `n` bases from a_at of the first read and from b_at of the second (offsets into the call's base arrays).
// Returns 0 (n may be 0: nothing to adjust) or the status both reads get.
__device__ int32_t pair_plan(const FinalizeParams &p, uint32_t i, uint32_t j, uint64_t *a_at, uint64_t *b_at, uint32_t *n) {
    *n = 0;
    if (!p.keep[i] || !p.keep[j]) return 0;
    uint32_t at[2] = {i, j};
    int64_t start[2], end[2], soft_start[2];
    const uint32_t *cig[2];
    uint32_t nc[2], flags[2];
    for (int k = 0; k < 2; ++k) {
        const uint32_t r = at[k];
        cig[k] = p.out_cigar + p.out_cigar_off[r];
        nc[k] = p.n_out_cigar[r];
        flags[k] = p.st_flags[r];
        start[k] = p.new_pos[r];
        int64_t ref_len = 0;
        soft_start[k] = start[k];
        bool leading = true;
        for (uint32_t c = 0; c < nc[k]; ++c) {
            const int op = op_of(cig[k][c]);
            ref_len += ref_len_of(cig[k][c]);
            if (leading && op == OP_S) soft_start[k] -= len_of(cig[k][c]);
            else if (op != OP_H) leading = false;
        }
        end[k] = start[k] + (ref_len > 0 ? ref_len - 1 : 0);
        const int64_t mpos = p.read_mpos[r];
        // fragment_collection.rs:47-51: this read won't overlap its mate, or doesn't have one
        if (!(flags[k] & FIN_FLAG_PAIRED) || (flags[k] & FIN_FLAG_MATE_UNMAPPED) || mpos == -1 || mpos > end[k]) return 0;
    }
    // which of the two the sorted order meets first: BirdToolRead::cmp (bird_tool_reads.rs:268-315) by the keys known here --
    // start, strand, flags, mapq, mpos, length -- then the lower index
    int first_met = 0;
    {
        const int64_t key[2][6] = {
            {start[0], (int64_t)((flags[0] >> 4) & 1u), (int64_t)(flags[0] & 0xffffu), (int64_t)((flags[0] >> 16) & 0xffu), p.read_mpos[i], (int64_t)p.clip_len[i]},
            {start[1], (int64_t)((flags[1] >> 4) & 1u), (int64_t)(flags[1] & 0xffffu), (int64_t)((flags[1] >> 16) & 0xffu), p.read_mpos[j], (int64_t)p.clip_len[j]}};
        for (int k = 0; k < 6; ++k)
            if (key[0][k] != key[1][k]) {
                first_met = key[0][k] < key[1][k] ? 0 : 1;
                break;
            }
    }
    // :33-38 the read with the smaller soft start is the first one; with equal soft starts the one met second
    if (soft_start[0] < 0 || soft_start[1] < 0) return FIN_ST_ARITHMETIC;   // get_soft_start().unwrap()
    const int a = soft_start[first_met] < soft_start[1 - first_met] ? first_met : 1 - first_met, b = 1 - a;
    if (end[a] < start[b]) return 0;   // fragments that do not overlap
    int64_t offset, first_end_base, second_end_base, second_offset;
    int op, unused;
    if (!read_index_for_reference_coordinate(soft_start[a], cig[a], nc[a], start[b], &offset, &op) || clipping(op)) return 0;
    if (!read_index_for_reference_coordinate(soft_start[a], cig[a], nc[a], end[a], &first_end_base, &unused) ||
        !read_index_for_reference_coordinate(soft_start[b], cig[b], nc[b], end[b], &second_end_base, &unused) ||
        !read_index_for_reference_coordinate(soft_start[b], cig[b], nc[b], start[b], &second_offset, &unused))
        return FIN_ST_PAIR;   // unwrap on None
    const int64_t da = first_end_base > offset ? first_end_base - offset : 0, db = second_end_base > second_offset ? second_end_base - second_offset : 0;
    const int64_t count = (da < db ? da : db) + 1;   // saturating_sub; + 1: R1 ending on the base R2 starts on is one base of overlap
    if (offset + count > (int64_t)p.clip_len[at[a]] || second_offset + count > (int64_t)p.clip_len[at[b]]) return FIN_ST_PAIR;   // index out of bounds
    *a_at = (uint64_t)p.read_off[at[a]] + p.clip_first[at[a]] + (uint64_t)offset;
    *b_at = (uint64_t)p.read_off[at[b]] + p.clip_first[at[b]] + (uint64_t)second_offset;
    *n = (uint32_t)count;
    return 0;
}

}  // namespace findev

}  // namespace phmm
