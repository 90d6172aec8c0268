// phmm_assembly_recover (include/phmm.h): dangling-end recovery -- recover_dangling_tails, then recover_dangling_heads
// (read_threading_graph.rs:779-1766 = R, base_graph.rs = B, abstract_read_threading_graph.rs:91-125, 202-212 = T) -- for many
// graphs in one launch.
//
// One workgroup of one wave per graph, graphs shared out over a grid that the aligner's slabs bound.  The wave keeps a working
// copy of the graph (its edges, then the edges it adds; its vertices, then the vertices an extension makes) and takes the ends
// STRICTLY one after the other, as the reference does: a merge changes degrees that a later end reads.
//   summaries   an edge-parallel pass over the working graph: degrees, the newest in- and out-edge (THE edge where the degree is
//               1), the oldest out-edge, reference bits, the newest reference out-edge, the newest in-edge from a reference node
//               (edges_directed lists the newest edge first: B:450-454, B:488-499).  Repeated after every end that changed the graph
//   an end      lane 0 walks (find_path, R:1651-1692), refuses (R:1386-1390, R:1453-1457), follows the reference path
//               (R:1556-1577) and writes the two strings (R:1735-1766); the wave fills the Smith-Waterman matrix of
//               smith_waterman_aligner.rs:124-271 one anti-diagonal per step (LeadingInDel: the edges carry gap penalties); lane 0
//               walks back (:273-443), drops a trailing deletion, tests the CIGAR and does the merge arithmetic
// n_rounds counts what the speculate-and-commit plan would have needed: an end that inspects a vertex whose edges an earlier
// end of the same round changed opens a new round.  Every walk is bounded by the vertices + 1, so a cyclic graph ends.
#include "phmm_recover_internal.hpp"

namespace phmm {
namespace {

constexpr int32_t SW_LOW_INIT = INT32_MIN / 2, SW_CUTOFF = -100000000;
enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2 };
enum { P_IN, P_OUT, P_INEDGE, P_OUTEDGE, P_OUTMIN, P_REF, P_REFOUT, P_PREVREF, P_MARK, P_TOUCHED };
static_assert(P_TOUCHED + 1 == RECOVER_VERTEX_WORDS, "planes");
enum { S_COUNT, S_GO, S_N, S_M, S_STATUS, S_CHANGED, S_WORDS };
// ONE wave per workgroup: between two barriers lane 0 writes words of s[] that the other lanes have read in the same
// instruction stream just before (S_N / S_M on the way of an end that is not aligned), which only program order protects
static_assert(RECOVER_THREADS == 64, "recover_kernel takes its workgroup to be one wavefront of 64 lanes");

__device__ __forceinline__ uint32_t ld(const uint32_t *at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct Work {  // the working graph of this wave and its slab
    uint32_t nv, ne, nvt, net, vcap, ecap, k, count, factor;
    uint32_t *pl[RECOVER_VERTEX_WORDS];
    uint32_t *src, *dst, *mult, *pmult;
    uint8_t *fl;
    const uint8_t *bases;
    const uint32_t *vbase;
    uint8_t *new_kmer;
    uint32_t kmer_stride;
    uint32_t *alt_path, *ref_path, *walk;
    uint8_t *alt_str, *ref_str;
    int32_t *diag[3], *lastcol, *bgv, *bgh, *gsv, *gsh;
    int16_t *bt;
    uint32_t cap_path, cap_str;
    __device__ uint8_t kb(uint32_t v, uint32_t i) const {
        return v < nv ? bases[vbase[v] + i] : new_kmer[(size_t)(v - nv) * kmer_stride + i];
    }
    __device__ bool is_ref_node(uint32_t v) const { return ld(pl[P_REF] + v) != 0 || count == 1; }             // B:130-146
    __device__ bool is_ref_source(uint32_t v) const {                                                            // B:339-360
        const uint32_t r = ld(pl[P_REF] + v);
        return r & 1 ? false : r & 2 ? true : count == 1;
    }
    __device__ bool is_ref_sink(uint32_t v) const {                                                              // B:366-387
        const uint32_t r = ld(pl[P_REF] + v);
        return r & 2 ? false : r & 1 ? true : count == 1;
    }
};

__device__ void summaries(const Work &w, uint32_t lane) {
    for (uint32_t v = lane; v < w.nvt; v += RECOVER_THREADS) {
        w.pl[P_IN][v] = w.pl[P_OUT][v] = w.pl[P_INEDGE][v] = w.pl[P_OUTEDGE][v] = w.pl[P_REF][v] = w.pl[P_REFOUT][v] = w.pl[P_PREVREF][v] = 0;
        w.pl[P_OUTMIN][v] = RECOVER_NONE;
    }
    __syncthreads();
    for (uint32_t e = lane; e < w.net; e += RECOVER_THREADS) {
        const uint8_t f = w.fl[e];
        if (f & RECOVER_EDGE_ABSENT) continue;
        const uint32_t a = w.src[e], b = w.dst[e];
        atomicAdd(w.pl[P_OUT] + a, 1u);
        atomicAdd(w.pl[P_IN] + b, 1u);
        atomicMax(w.pl[P_INEDGE] + b, e + 1);
        atomicMax(w.pl[P_OUTEDGE] + a, e + 1);
        atomicMin(w.pl[P_OUTMIN] + a, e + 1);
        if (f & RECOVER_EDGE_REF) {
            atomicOr(w.pl[P_REF] + a, 2u);
            atomicOr(w.pl[P_REF] + b, 1u);
            atomicMax(w.pl[P_REFOUT] + a, e + 1);
        }
    }
    __syncthreads();
    for (uint32_t e = lane; e < w.net; e += RECOVER_THREADS) {
        if (w.fl[e] & RECOVER_EDGE_ABSENT) continue;
        if (w.is_ref_node(w.src[e])) atomicMax(w.pl[P_PREVREF] + w.dst[e], e + 1);
    }
    __syncthreads();
}

// smith_waterman_aligner.rs:124-271 with OverhangStrategy::LeadingInDel, one anti-diagonal per step: cell (i, d - i) reads the
// diagonals d - 1 and d - 2 and its own column's and row's best gap, which the cell before it on that column / row left
__device__ void fill_matrix(const Work &w, uint32_t lane, int n, int m, int32_t wm, int32_t wx, int32_t wo, int32_t we) {
    for (int i = lane; i <= n + 1; i += RECOVER_THREADS) {
        w.bgh[i] = SW_LOW_INIT;
        w.gsh[i] = 0;
        w.lastcol[i] = 0;
    }
    for (int j = lane; j <= m + 1; j += RECOVER_THREADS) {
        w.bgv[j] = SW_LOW_INIT;
        w.gsv[j] = 0;
    }
    __syncthreads();
    auto edge = [&](int i, int j) -> int32_t { return i == 0 && j == 0 ? 0 : wo + ((i == 0 ? j : i) - 1) * we; };   // :145-178
    const size_t ncol = (size_t)m + 1;
    for (int d = 2; d <= n + m; ++d) {
        int32_t *const cur = w.diag[d % 3];
        const int32_t *const p1 = w.diag[(d - 1) % 3], *const p2 = w.diag[(d - 2) % 3];
        const int ilo = d - m > 1 ? d - m : 1, ihi = d - 1 < n ? d - 1 : n;
        for (int i = ilo + (int)lane; i <= ihi; i += RECOVER_THREADS) {
            const int j = d - i;
            const int32_t sw_diag = i > 1 && j > 1 ? p2[i - 1] : edge(i - 1, j - 1);
            const int32_t sw_up = i > 1 ? p1[i - 1] : edge(0, j), sw_left = j > 1 ? p1[i] : edge(i, 0);
            const int32_t step_diag = sw_diag + (w.ref_str[i - 1] == w.alt_str[j - 1] ? wm : wx);      // :194-199
            int32_t prev_gap = sw_up + wo, bv = w.bgv[j] + we, kd;                                      // :207-218
            if (prev_gap > bv) {
                bv = prev_gap;
                kd = 1;
            } else {
                kd = w.gsv[j] + 1;
            }
            w.bgv[j] = bv;
            w.gsv[j] = kd;
            int32_t bh = w.bgh[i] + we, ki;                                                             // :229-240
            prev_gap = sw_left + wo;
            if (prev_gap > bh) {
                bh = prev_gap;
                ki = 1;
            } else {
                ki = w.gsh[i] + 1;
            }
            w.bgh[i] = bh;
            w.gsh[i] = ki;
            int32_t val, bt;                                                                            // :250-266
            if (step_diag >= bv && step_diag >= bh) {
                val = step_diag;
                bt = 0;
            } else if (bh >= bv) {
                val = bh;
                bt = -ki;
            } else {
                val = bv;
                bt = kd;
            }
            val = val > SW_CUTOFF ? val : SW_CUTOFF;
            cur[i] = val;
            w.bt[(size_t)i * ncol + j] = (int16_t)bt;
            if (j == m) w.lastcol[i] = val;
        }
        __syncthreads();
    }
}

struct Cigar {  // of an end, front to back, a trailing deletion removed (alignment_utils.rs:702-707)
    uint32_t n, ref_len, read_len, el[RECOVER_CIGAR_SHOWN];
    __device__ uint32_t op(uint32_t i) const { return el[i] & 15u; }
    __device__ uint32_t len(uint32_t i) const { return el[i] >> 4; }
};

// :273-443 for LeadingInDel: the best cell of the last column (`>=`: of equal scores the LAST row scanned, the highest index,
// :303-309), the walk, the leading gap
__device__ Cigar walk_back(const Work &w, int n, int m) {
    int p1 = 0, p2 = m;
    int32_t best = INT32_MIN;
    for (int i = 1; i <= n; ++i)
        if (w.lastcol[i] >= best) {
            best = w.lastcol[i];
            p1 = i;
        }
    uint32_t c = 0, ring[4] = {0, 0, 0, 0}, first2[2] = {0, 0}, ref_len = 0, read_len = 0;
    auto push = [&](uint32_t op, uint32_t len) {
        const uint32_t e = (len << 4) | op;
        if (c < 2) first2[c] = e;
        ring[c & 3] = e;
        ++c;
        if (op != OP_I) ref_len += len;
        if (op != OP_D) read_len += len;
    };
    uint32_t state = OP_M;
    int32_t segment_length = 0;
    const size_t ncol = (size_t)m + 1;
    for (;;) {
        const int32_t btr = w.bt[(size_t)p1 * ncol + p2];
        uint32_t new_state = OP_M;
        int32_t step_length = 1;
        if (btr > 0) {
            new_state = OP_D;
            step_length = btr;
            p1 -= step_length;
        } else if (btr < 0) {
            new_state = OP_I;
            step_length = -btr;
            p2 -= step_length;
        } else {
            --p1;
            --p2;
        }
        if (new_state == state) {
            segment_length += step_length;
        } else {
            if (segment_length > 0) push(state, (uint32_t)segment_length);
            segment_length = step_length;
            state = new_state;
        }
        if (p1 <= 0 || p2 <= 0) break;
    }
    push(state, (uint32_t)segment_length);
    if (p1 > 0) push(OP_D, (uint32_t)p1);
    else if (p2 > 0) push(OP_I, (uint32_t)p2);
    Cigar out;
    out.n = c;
    out.ref_len = ref_len;
    out.read_len = read_len;
    if ((first2[0] & 15u) == OP_D) {  // pushed first = the last element
        out.n = c - 1;
        out.ref_len -= first2[0] >> 4;
    }
    for (uint32_t i = 0; i < RECOVER_CIGAR_SHOWN; ++i) out.el[i] = i < out.n ? ring[(c - 1 - i) & 3] : 0u;
    return out;
}

__global__ __launch_bounds__(RECOVER_THREADS) void recover_kernel(RecoverParams p) {
    const uint32_t lane = threadIdx.x;
    __shared__ uint32_t s[S_WORDS];
    Work w;
    {  // the slab of this workgroup
        unsigned char *at = p.slab + (size_t)blockIdx.x * p.slab_stride;
        const size_t L = p.slab_len;
        w.alt_path = (uint32_t *)at;
        w.ref_path = w.alt_path + (L + 1);
        w.walk = w.ref_path + (L + 1);
        int32_t *rows = (int32_t *)(w.walk + (L + 1));
        for (int i = 0; i < 3; ++i) w.diag[i] = rows + (size_t)i * (L + 2);
        w.lastcol = rows + 3 * (L + 2);
        w.bgv = rows + 4 * (L + 2);
        w.bgh = rows + 5 * (L + 2);
        w.gsv = rows + 6 * (L + 2);
        w.gsh = rows + 7 * (L + 2);
        w.alt_str = (uint8_t *)(rows + 8 * (L + 2));
        w.ref_str = w.alt_str + (L + 4) / 4 * 4;
        w.bt = (int16_t *)(w.ref_str + (L + 4) / 4 * 4);
    }
    w.bases = p.bases;
    w.kmer_stride = p.kmer_stride;
    for (uint32_t g = blockIdx.x; g < p.n_graphs; g += gridDim.x) {
        const uint32_t v0 = p.vertex_off[g], e0 = p.edge_off[g], xv0 = p.xv_off[g], xe0 = p.xe_off[g];
        w.nv = w.nvt = p.vertex_off[g + 1] - v0;
        w.ne = w.net = p.edge_off[g + 1] - e0;
        w.vcap = p.xv_off[g + 1] - xv0;
        w.ecap = p.xe_off[g + 1] - xe0;
        w.k = p.k[g / p.n_regions];
        w.factor = p.prune_factor[g];
        for (int i = 0; i < RECOVER_VERTEX_WORDS; ++i) w.pl[i] = p.xv + (size_t)i * p.xv_total + xv0;
        w.src = p.xe_src + xe0;
        w.dst = p.xe_dst + xe0;
        w.mult = p.xe_mult + xe0;
        w.pmult = p.xe_pmult + xe0;
        w.fl = p.xe_flags + xe0;
        w.vbase = p.vertex_base + v0;
        w.new_kmer = p.new_kmer + (size_t)(xv0 - v0) * p.kmer_stride;
        w.cap_path = p.slab_len - w.k - 1;
        w.cap_str = p.slab_len;
        uint8_t *const vabs = p.xv_absent + xv0;
        uint32_t *const ne_src = p.ne_src + (xe0 - e0), *const ne_dst = p.ne_dst + (xe0 - e0), *const ne_mult = p.ne_mult + (xe0 - e0),
                       *const ne_pmult = p.ne_pmult + (xe0 - e0);
        const uint32_t end0 = p.xend_off[g], end_cap = p.xend_off[g + 1] - end0;
        uint32_t *const end_vertex = p.end_vertex + end0;

        if (end_cap == 0) {  // no vertex the host's degree pass could take for an end: nothing to copy, nothing to walk
            for (uint32_t e = lane; e < w.ne; e += RECOVER_THREADS) p.edge_removed[e0 + e] = 0;
            if (lane < 8) p.g_counts[(size_t)g * 8 + lane] = 0;
            continue;
        }
        // ---- the working copy ----------------------------------------------------------------------------------------------
        if (lane == 0) s[S_COUNT] = 0;
        __syncthreads();
        uint32_t present = 0;
        for (uint32_t v = lane; v < w.vcap; v += RECOVER_THREADS) {
            const bool absent = v < w.nv && p.vertex_absent && p.vertex_absent[v0 + v];
            vabs[v] = absent;
            present += v < w.nv && !absent;
            w.pl[P_MARK][v] = w.pl[P_TOUCHED][v] = 0;
        }
        if (present) atomicAdd(&s[S_COUNT], present);
        for (uint32_t e = lane; e < w.ne; e += RECOVER_THREADS) {
            w.src[e] = p.edge_src[e0 + e];
            w.dst[e] = p.edge_dst[e0 + e];
            w.mult[e] = p.edge_mult[e0 + e];
            w.pmult[e] = p.edge_pmult[e0 + e];
            w.fl[e] = (p.edge_absent && p.edge_absent[e0 + e] ? RECOVER_EDGE_ABSENT : 0) | (p.edge_is_ref[e0 + e] ? RECOVER_EDGE_REF : 0);
            p.edge_removed[e0 + e] = 0;
        }
        __syncthreads();
        w.count = s[S_COUNT];

        uint32_t n_ends = 0, n_rounds = 0, stamp = 0, round = 0;
        uint32_t tally[4] = {0, 0, 0, 0};  // tails, tails recovered, heads, heads recovered
        for (uint32_t kind = RECOVER_TAIL; kind <= RECOVER_HEAD; ++kind) {
            if (!(p.ops & (kind == RECOVER_TAIL ? RECOVER_OP_TAILS : RECOVER_OP_HEADS))) continue;
            summaries(w, lane);
            // ---- the ends of this kind, in NodeIndex order, listed before any is touched (R:792-797, R:837-842) ---------------
            const uint32_t first_end = n_ends;
            for (uint32_t vb = 0; vb < w.nvt; vb += RECOVER_THREADS) {
                const uint32_t v = vb + lane;
                bool is = false;
                if (v < w.nvt && !vabs[v])
                    is = kind == RECOVER_TAIL ? ld(w.pl[P_OUT] + v) == 0 && !w.is_ref_sink(v) : ld(w.pl[P_IN] + v) == 0 && !w.is_ref_source(v);
                const uint64_t m = __ballot(is);
                const uint32_t at = n_ends + __popcll(m & ((1ull << lane) - 1ull));
                if (is && at < end_cap) end_vertex[at] = v;
                n_ends += __popcll(m);
            }
            if (n_ends > end_cap) n_ends = end_cap;  // (the host counted: cannot happen)
            __syncthreads();
            if (n_ends > first_end) {
                ++n_rounds;
                ++round;
            }
            for (uint32_t ei = first_end; ei < n_ends; ++ei) {
                const uint32_t vertex = end_vertex[ei];
                ++stamp;
                // ---- lane 0: the walk, the refusals, the reference path, the strings ------------------------------------------
                if (lane == 0) {
                    uint32_t status = RECOVER_NONE, v = vertex, n_walk = 0, steps = 0, n_alt = 0, n_ref = 0, n = 0, m = 0;
                    bool touched = false;
                    auto look = [&](uint32_t x) { touched |= w.pl[P_TOUCHED][x] == round; };
                    const bool tail = kind == RECOVER_TAIL;
                    for (;;) {  // find_path, R:1651-1692 with the closures of R:1596-1605 / R:1506-1515
                        look(v);
                        const uint32_t din = ld(w.pl[P_IN] + v), dout = ld(w.pl[P_OUT] + v);
                        const bool done = tail ? din != 1 || dout >= 2 : w.is_ref_node(v) || dout != 1;
                        if (done) break;
                        const uint32_t e = ld(w.pl[tail ? P_INEDGE : P_OUTEDGE] + v) - 1;
                        if (w.pmult[e] < w.factor) {  // R:1667-1677: the marks stay, they are visited_nodes
                            n_walk = 0;
                        } else {
                            if (n_walk + 1 >= w.cap_path) {
                                status = RECOVER_REFERENCE_FAILS;
                                break;
                            }
                            w.walk[n_walk++] = v;
                            w.pl[P_MARK][v] = stamp;
                        }
                        v = tail ? w.src[e] : w.dst[e];
                        if (w.pl[P_MARK][v] == stamp) {  // R:1684-1687
                            status = RECOVER_LOOP;
                            break;
                        }
                        if (++steps > w.nvt) {  // a ring of low edges: the reference rides forever
                            status = RECOVER_REFERENCE_FAILS;
                            break;
                        }
                    }
                    if (status == RECOVER_NONE) {
                        const bool give = tail ? ld(w.pl[P_OUT] + v) > 1 : w.is_ref_node(v);  // return_path
                        if (!give) status = RECOVER_NO_PATH;
                    }
                    if (status == RECOVER_NONE) {
                        n_alt = n_walk + 1;
                        w.alt_path[0] = v;
                        for (uint32_t i = 1; i < n_alt; ++i) w.alt_path[i] = w.walk[n_walk - i];
                        const int32_t min_len = tail ? (p.min_dangling_branch_length > 1 ? p.min_dangling_branch_length : 1) : p.min_dangling_branch_length;
                        if (tail ? w.is_ref_source(v) : w.is_ref_sink(v)) status = RECOVER_AT_REF_END;          // R:1386, R:1453
                        else if ((int64_t)n_alt < (int64_t)min_len + 1) status = RECOVER_TOO_SHORT;            // R:1387, R:1454
                    }
                    if (status == RECOVER_NONE) {  // get_reference_path, R:1556-1577
                        const uint32_t blacklisted = tail ? ld(w.pl[P_INEDGE] + w.alt_path[1]) - 1 : RECOVER_NONE;   // R:1399
                        for (uint32_t x = w.alt_path[0]; x != RECOVER_NONE;) {
                            if (n_ref > w.nvt || n_ref >= w.cap_path) {  // a cycle: the reference never returns
                                status = RECOVER_REFERENCE_FAILS;
                                break;
                            }
                            w.ref_path[n_ref++] = x;
                            look(x);
                            if (tail) {  // B:437-481
                                const uint32_t ro = ld(w.pl[P_REFOUT] + x);
                                if (ro) {
                                    x = w.dst[ro - 1];
                                } else {
                                    const uint32_t dout = ld(w.pl[P_OUT] + x);
                                    const bool mine = blacklisted != RECOVER_NONE && w.src[blacklisted] == x;
                                    if (dout - (mine ? 1u : 0u) != 1u) {
                                        x = RECOVER_NONE;
                                    } else {
                                        uint32_t e = ld(w.pl[P_OUTEDGE] + x) - 1;
                                        if (mine && e == blacklisted) e = ld(w.pl[P_OUTMIN] + x) - 1;
                                        x = w.dst[e];
                                    }
                                }
                            } else {  // B:488-499
                                const uint32_t pr = ld(w.pl[P_PREVREF] + x);
                                x = pr ? w.src[pr - 1] : RECOVER_NONE;
                            }
                        }
                    }
                    if (status == RECOVER_NONE) {  // get_bases_for_path, R:1735-1766
                        for (int which = 0; which < 2 && status == RECOVER_NONE; ++which) {
                            const uint32_t *path = which ? w.alt_path : w.ref_path;
                            uint8_t *str = which ? w.alt_str : w.ref_str;
                            const uint32_t np = which ? n_alt : n_ref;
                            uint32_t at = 0;
                            for (uint32_t i = 0; i < np; ++i) {
                                const uint32_t x = path[i];
                                const bool expand = !tail && ld(w.pl[P_IN] + x) == 0;
                                if (at + (expand ? w.k : 1u) > w.cap_str) {
                                    status = RECOVER_REFERENCE_FAILS;
                                    break;
                                }
                                if (expand)
                                    for (uint32_t t = 0; t < w.k; ++t) str[at++] = w.kb(x, w.k - 1 - t);
                                else
                                    str[at++] = w.kb(x, w.k - 1);
                            }
                            (which ? m : n) = at;
                        }
                    }
                    if (touched) {  // the plan would have stopped this graph's round here and taken the end up again in the next
                        ++n_rounds;
                        ++round;
                    }
                    s[S_GO] = status == RECOVER_NONE;
                    s[S_N] = n;
                    s[S_M] = m;
                    s[S_STATUS] = status;
                    s[S_CHANGED] = 0;
                    // (for the commit below)
                    w.walk[0] = n_alt;
                    w.walk[1] = n_ref;
                }
                __syncthreads();
                n_rounds = __shfl(n_rounds, 0);
                round = __shfl(round, 0);
                const bool go = s[S_GO];
                const int n = (int)s[S_N], m = (int)s[S_M];
                if (go) fill_matrix(w, lane, n, m, p.w_match, p.w_mismatch, p.w_open, p.w_extend);
                // ---- lane 0: the CIGAR, the tests, the merge ----------------------------------------------------------------------
                if (lane == 0) {
                    uint32_t status = s[S_STATUS], made_edge = RECOVER_NONE;
                    Cigar c{};
                    bool changed = false;
                    auto touch = [&](uint32_t x) { w.pl[P_TOUCHED][x] = round; };
                    auto add_edge = [&](uint32_t a, uint32_t b, uint32_t multiplicity) {  // multi_sample_edge.rs:119-131: a heap of one
                        const uint32_t e = w.net++;
                        w.src[e] = a;
                        w.dst[e] = b;
                        w.mult[e] = w.pmult[e] = multiplicity;
                        w.fl[e] = 0;
                        touch(a);
                        touch(b);
                        changed = true;
                        return e - w.ne;
                    };
                    if (go) {
                        uint32_t n_alt = w.walk[0];
                        const uint32_t n_ref = w.walk[1];
                        c = walk_back(w, n, m);
                        const bool tail = kind == RECOVER_TAIL;
                        const bool okay = c.n != 0 && c.n <= 3 && (tail ? c.op(c.n - 1) == OP_M : c.op(0) == OP_M);   // T:91-125, R:69
                        if (!okay) {
                            status = RECOVER_CIGAR_NOT_OKAY;
                        } else if (tail) {  // merge_dangling_tail, R:961-1036
                            const int64_t last_ref_index = (int64_t)c.ref_len - 1;
                            int64_t matching_suffix = m;  // longest_suffix_match, T:202-212
                            for (int64_t len = 1; len <= m; ++len) {
                                const int64_t seq_i = last_ref_index - len + 1, kmer_i = m - len;
                                if (seq_i < 0 || w.ref_str[seq_i] != w.alt_str[kmer_i]) {
                                    matching_suffix = len - 1;
                                    break;
                                }
                            }
                            if (matching_suffix > (int64_t)c.len(c.n - 1)) matching_suffix = c.len(c.n - 1);
                            const bool few = p.min_matching_bases >= 0 ? matching_suffix < p.min_matching_bases : matching_suffix == 0;
                            int64_t alt_index = (int64_t)c.read_len - matching_suffix;
                            alt_index = (alt_index > 0 ? alt_index : 0) - 1;
                            if (alt_index < 0) alt_index = 0;
                            const bool leading = c.op(0) == OP_D && (int64_t)c.len(0) + matching_suffix == last_ref_index + 1;
                            const int64_t ref_index = last_ref_index - matching_suffix + 1 + (leading ? 1 : 0);
                            if (few) status = RECOVER_TOO_FEW_MATCHING;
                            else if (ref_index <= 0) status = RECOVER_WHOLE_INSERTION;
                            else if (ref_index >= (int64_t)n_ref || alt_index >= (int64_t)n_alt || w.net >= w.ecap) status = RECOVER_REFERENCE_FAILS;
                            else {
                                made_edge = add_edge(w.alt_path[alt_index], w.ref_path[ref_index], 1u);
                                status = RECOVER_MERGED;
                            }
                        } else {
                            int64_t i0 = -1, i1 = -1;
                            if (p.min_matching_bases >= 0) {  // best_prefix_match, R:1303-1351
                                int64_t ref_idx = (int64_t)c.ref_len - 1, read_idx = (int64_t)m - 1;
                                bool stop = false;
                                for (int q = (int)c.n - 1; q >= 0 && !stop; --q) {
                                    if (c.op(q) != OP_M) break;
                                    for (uint32_t j = 0; j < c.len(q); ++j) {
                                        if (w.ref_str[ref_idx] != w.alt_str[read_idx]) {
                                            stop = true;
                                            break;
                                        }
                                        --ref_idx;
                                        --read_idx;
                                        if (ref_idx < 0 || read_idx < 0) {
                                            stop = true;
                                            break;
                                        }
                                    }
                                }
                                const int64_t matches = (int64_t)m - 1 - read_idx;
                                if (matches < p.min_matching_bases) status = RECOVER_TOO_FEW_MATCHING;
                                else if (ref_idx <= 0 || read_idx <= 0) status = RECOVER_NO_MERGE_POINT;          // R:1179-1181
                                else if (ref_idx >= (int64_t)n_ref - 1) status = RECOVER_CANNOT_PUSH_REF;         // R:1184-1186
                                i0 = ref_idx;
                                i1 = read_idx;
                            } else {  // best_prefix_match_legacy, R:1106-1151
                                const int64_t max_index = c.len(0);
                                int64_t max_mismatches = p.max_mismatches_in_dangling_head > 0 ? p.max_mismatches_in_dangling_head : max_index / (int64_t)w.k;
                                if (p.max_mismatches_in_dangling_head <= 0 && max_mismatches < 1) max_mismatches = 1;
                                int64_t mismatches = 0, last_good = -1;
                                status = RECOVER_NO_MERGE_POINT;
                                for (int64_t index = 0; index < max_index; ++index)
                                    if (w.ref_str[index] != w.alt_str[index]) {
                                        if (++mismatches > max_mismatches) {
                                            status = RECOVER_TOO_MANY_MISMATCHES;
                                            last_good = -1;
                                            break;
                                        }
                                        last_good = index;
                                    }
                                if (last_good >= 0) status = last_good >= (int64_t)n_ref - 1 ? RECOVER_CANNOT_PUSH_REF : RECOVER_NONE;   // R:1068-1070
                                i0 = i1 = last_good;
                            }
                            if (status == RECOVER_NONE) {
                                const int64_t num = i1 - (int64_t)n_alt + 2;                                     // R:1189-1190, R:1073-1074
                                if (i1 >= (int64_t)n_alt) {  // extend_dangling_path_against_reference, R:1209-1291
                                    const int64_t index_of_last = (int64_t)n_alt - 1;
                                    const int64_t iref = index_of_last + ((int64_t)c.ref_len - (int64_t)c.read_len) + num;
                                    if (iref >= (int64_t)n_ref || iref < 0) {
                                        status = RECOVER_CANNOT_EXTEND;
                                    } else if (w.net + num + 1 > w.ecap || w.nvt + num > w.vcap || num > (int64_t)w.k) {
                                        status = RECOVER_REFERENCE_FAILS;  // (the host sized the slots for k vertices per head: cannot happen)
                                    } else {
                                        const uint32_t dangling_source = w.alt_path[index_of_last], ref_v = w.ref_path[iref];
                                        uint32_t source_edge = RECOVER_NONE;  // get_heaviest_edge, R:1703-1726: the oldest of the heaviest
                                        if (ld(w.pl[P_OUT] + dangling_source) == 1) {
                                            source_edge = ld(w.pl[P_OUTEDGE] + dangling_source) - 1;
                                        } else {
                                            for (uint32_t e = 0; e < w.net; ++e)
                                                if (!(w.fl[e] & RECOVER_EDGE_ABSENT) && w.src[e] == dangling_source &&
                                                    (source_edge == RECOVER_NONE || w.mult[e] > w.mult[source_edge]))
                                                    source_edge = e;
                                        }
                                        if (source_edge == RECOVER_NONE) {
                                            status = RECOVER_REFERENCE_FAILS;
                                        } else {
                                            uint32_t prev_v = w.dst[source_edge];
                                            const uint32_t multiplicity = w.mult[source_edge];
                                            w.fl[source_edge] |= RECOVER_EDGE_ABSENT;                            // R:1274
                                            if (source_edge < w.ne) p.edge_removed[e0 + source_edge] = 1;
                                            touch(dangling_source);
                                            touch(prev_v);
                                            --n_alt;
                                            for (int64_t i = num; i >= 1; --i) {                                 // R:1278-1288
                                                const uint32_t new_v = w.nvt;
                                                uint8_t *kmer = w.new_kmer + (size_t)(new_v - w.nv) * w.kmer_stride;
                                                for (uint32_t t = 0; t < w.k; ++t)
                                                    kmer[t] = i + t < num ? w.kb(ref_v, (uint32_t)(i + t)) : w.kb(dangling_source, (uint32_t)(i + t - num));
                                                vabs[new_v] = 0;
                                                ++w.nvt;
                                                ++w.count;
                                                (void)add_edge(new_v, prev_v, multiplicity);
                                                w.alt_path[n_alt++] = new_v;
                                                prev_v = new_v;
                                            }
                                        }
                                    }
                                }
                                if (status == RECOVER_NONE) {
                                    if (w.net >= w.ecap || i1 >= (int64_t)n_alt) {
                                        status = RECOVER_REFERENCE_FAILS;
                                    } else {
                                        made_edge = add_edge(w.ref_path[i0 + 1], w.alt_path[i1], 1u);           // R:1200-1204, R:1086-1090
                                        status = RECOVER_MERGED;
                                    }
                                }
                            }
                        }
                    }
                    const uint32_t at = end0 + ei;
                    p.end_kind[at] = kind;
                    p.end_status[at] = status;
                    p.end_alt_len[at] = go ? (uint32_t)m : 0u;
                    p.end_ref_len[at] = go ? (uint32_t)n : 0u;
                    p.end_n_cigar[at] = c.n;
                    for (uint32_t i = 0; i < RECOVER_CIGAR_SHOWN; ++i) p.end_cigar[(size_t)at * RECOVER_CIGAR_SHOWN + i] = c.el[i];
                    p.end_edge[at] = made_edge;
                    s[S_CHANGED] = changed;
                    s[S_STATUS] = status;
                    s[S_N] = w.nvt;
                    s[S_M] = w.net;
                    s[S_COUNT] = w.count;
                }
                __syncthreads();
                w.nvt = s[S_N];
                w.net = s[S_M];
                w.count = s[S_COUNT];
                tally[2 * kind] += 1;
                tally[2 * kind + 1] += s[S_STATUS] == RECOVER_MERGED;
                const bool changed = s[S_CHANGED];
                __syncthreads();
                if (changed) summaries(w, lane);
            }
        }
        // ---- what the graph gained ----------------------------------------------------------------------------------------
        for (uint32_t e = w.ne + lane; e < w.net; e += RECOVER_THREADS) {
            const bool gone = w.fl[e] & RECOVER_EDGE_ABSENT;  // a new edge that a later extension took out again: vacant
            ne_src[e - w.ne] = gone ? RECOVER_NONE : w.src[e];
            ne_dst[e - w.ne] = gone ? RECOVER_NONE : w.dst[e];
            ne_mult[e - w.ne] = w.mult[e];
            ne_pmult[e - w.ne] = w.pmult[e];
        }
        if (lane < 8) {
            const uint32_t vals[8] = {tally[0], tally[1], tally[2], tally[3], w.net - w.ne, w.nvt - w.nv, n_rounds, n_ends};
            p.g_counts[(size_t)g * 8 + lane] = vals[lane];
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_recover(const RecoverParams &p, uint32_t n_blocks, hipStream_t stream) {
    if (!p.n_graphs || !n_blocks) return hipSuccess;
    hipLaunchKernelGGL(recover_kernel, dim3(n_blocks), dim3(RECOVER_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace phmm
