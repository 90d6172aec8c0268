// A plain single-threaded host loop over the arrays phmm_assembly_recover takes: what tools/assembly_recover_bench.py times
// beside the device call, for scale and not as a gate, and compares with it for equality.  Per graph: summaries over the edges
// (degrees, the newest and the oldest edge per vertex, reference bits, the newest reference neighbours), the ends one after the
// other -- the walk, the refusals, the reference path, the two strings, a full-matrix Smith-Waterman with LeadingInDel, the
// walk back, the merge arithmetic -- and the summaries again after every end that changed the graph.  No device code.
// `bases` holds every sequence's bytes and vertex_base[v] where vertex v's k bytes start in it (the caller's arithmetic).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

constexpr uint32_t NONE = 0xffffffffu;
enum : uint32_t { NO_PATH, LOOP, AT_REF_END, TOO_SHORT, CIGAR_NOT_OKAY, TOO_FEW_MATCHING, WHOLE_INSERTION, TOO_MANY_MISMATCHES, CANNOT_PUSH_REF,
                  CANNOT_EXTEND, MERGED, NO_MERGE_POINT, REFERENCE_FAILS };
enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2 };

struct Graph {
    uint32_t nv = 0, k = 0, count = 0;
    std::vector<uint32_t> src, dst, mult, pmult;
    std::vector<uint8_t> gone, is_ref;
    std::vector<std::vector<uint8_t>> new_kmer;
    const uint8_t *bases = nullptr;
    const uint32_t *vbase = nullptr;
    // summaries
    std::vector<uint32_t> din, dout, in_edge, out_edge, out_min, ref, ref_out, prev_ref;
    uint32_t nvt() const { return nv + (uint32_t)new_kmer.size(); }
    uint8_t kb(uint32_t v, uint32_t i) const { return v < nv ? bases[vbase[v] + i] : new_kmer[v - nv][i]; }
    bool is_ref_node(uint32_t v) const { return ref[v] != 0 || count == 1; }
    bool is_ref_source(uint32_t v) const { return ref[v] & 1 ? false : ref[v] & 2 ? true : count == 1; }
    bool is_ref_sink(uint32_t v) const { return ref[v] & 2 ? false : ref[v] & 1 ? true : count == 1; }
    void summaries() {
        const uint32_t n = nvt();
        din.assign(n, 0), dout.assign(n, 0), in_edge.assign(n, 0), out_edge.assign(n, 0), out_min.assign(n, NONE), ref.assign(n, 0), ref_out.assign(n, 0), prev_ref.assign(n, 0);
        for (uint32_t e = 0; e < src.size(); ++e) {
            if (gone[e]) continue;
            const uint32_t a = src[e], b = dst[e];
            ++dout[a], ++din[b];
            in_edge[b] = e + 1, out_edge[a] = e + 1;  // ascending: the newest stays
            if (out_min[a] == NONE) out_min[a] = e + 1;
            if (is_ref[e]) ref[a] |= 2, ref[b] |= 1, ref_out[a] = e + 1;
        }
        for (uint32_t e = 0; e < src.size(); ++e)
            if (!gone[e] && is_ref_node(src[e])) prev_ref[dst[e]] = e + 1;
    }
    uint32_t add_edge(uint32_t a, uint32_t b, uint32_t m) {
        src.push_back(a), dst.push_back(b), mult.push_back(m), pmult.push_back(m), gone.push_back(0), is_ref.push_back(0);
        return (uint32_t)src.size() - 1;
    }
};

struct Cigar {
    std::vector<uint32_t> el;  // front to back, the trailing deletion removed
    uint32_t ref_len = 0, read_len = 0;
};

Cigar align(const std::vector<uint8_t> &r, const std::vector<uint8_t> &a, const int32_t w[4]) {
    const int n = (int)r.size(), m = (int)a.size();
    const size_t nc = (size_t)m + 1;
    std::vector<int32_t> sw((size_t)(n + 1) * nc, 0), bt((size_t)(n + 1) * nc, 0), bgv(m + 2, INT32_MIN / 2), gsv(m + 2, 0), bgh(n + 2, INT32_MIN / 2), gsh(n + 2, 0);
    for (int j = 1; j <= m; ++j) sw[j] = w[2] + (j - 1) * w[3];
    for (int i = 1; i <= n; ++i) sw[i * nc] = w[2] + (i - 1) * w[3];
    for (int i = 1; i <= n; ++i)
        for (int j = 1; j <= m; ++j) {
            const int32_t step_diag = sw[(i - 1) * nc + j - 1] + (r[i - 1] == a[j - 1] ? w[0] : w[1]);
            int32_t prev_gap = sw[(i - 1) * nc + j] + w[2];
            bgv[j] += w[3];
            if (prev_gap > bgv[j]) bgv[j] = prev_gap, gsv[j] = 1;
            else ++gsv[j];
            prev_gap = sw[i * nc + j - 1] + w[2];
            bgh[i] += w[3];
            if (prev_gap > bgh[i]) bgh[i] = prev_gap, gsh[i] = 1;
            else ++gsh[i];
            int32_t val, b;
            if (step_diag >= bgv[j] && step_diag >= bgh[i]) val = step_diag, b = 0;
            else if (bgh[i] >= bgv[j]) val = bgh[i], b = -gsh[i];
            else val = bgv[j], b = gsv[j];
            sw[i * nc + j] = std::max(val, -100000000);
            bt[i * nc + j] = b;
        }
    int p1 = 0, p2 = m;
    int32_t best = INT32_MIN;
    for (int i = 1; i <= n; ++i)
        if (sw[i * nc + m] >= best) best = sw[i * nc + m], p1 = i;
    std::vector<uint32_t> back;
    uint32_t state = OP_M;
    int32_t seg = 0;
    for (;;) {
        const int32_t b = bt[p1 * nc + p2];
        uint32_t ns = OP_M;
        int32_t step = 1;
        if (b > 0) ns = OP_D, step = b, p1 -= step;
        else if (b < 0) ns = OP_I, step = -b, p2 -= step;
        else --p1, --p2;
        if (ns == state) seg += step;
        else {
            if (seg > 0) back.push_back(((uint32_t)seg << 4) | state);
            seg = step, state = ns;
        }
        if (p1 <= 0 || p2 <= 0) break;
    }
    back.push_back(((uint32_t)seg << 4) | state);
    if (p1 > 0) back.push_back(((uint32_t)p1 << 4) | OP_D);
    else if (p2 > 0) back.push_back(((uint32_t)p2 << 4) | OP_I);
    Cigar c;
    c.el.assign(back.rbegin(), back.rend());
    if ((c.el.back() & 15u) == OP_D) c.el.pop_back();
    for (uint32_t e : c.el) {
        if ((e & 15u) != OP_I) c.ref_len += e >> 4;
        if ((e & 15u) != OP_D) c.read_len += e >> 4;
    }
    return c;
}

}  // namespace

extern "C" int assembly_recover_host(
    uint32_t n_graphs, uint32_t n_regions, const uint32_t *k, const uint8_t *bases, const uint32_t *vertex_base, const uint32_t *vertex_off,
    const uint32_t *edge_off, const uint32_t *edge_src, const uint32_t *edge_dst, const uint8_t *edge_is_ref, const uint32_t *edge_mult,
    const uint32_t *edge_pmult, const uint8_t *vertex_absent, const uint8_t *edge_absent, const uint32_t *prune_factor, uint32_t ops,
    int32_t min_dangling_branch_length, int32_t min_matching_bases, int32_t max_mismatches, const int32_t *weights, uint32_t kmer_stride,
    const uint32_t *capacity, uint32_t *counts /* [n_graphs][6] */, uint32_t *end_off, uint32_t *new_edge_off, uint32_t *new_vertex_off,
    uint32_t *end_vertex, uint32_t *end_kind, uint32_t *end_status, uint32_t *end_alt_len, uint32_t *end_ref_len, uint32_t *end_n_cigar,
    uint32_t *end_cigar, uint32_t *end_edge, uint32_t *ne_src, uint32_t *ne_dst, uint32_t *ne_mult, uint32_t *ne_pmult, uint8_t *new_kmer,
    uint8_t *edge_removed) {
    uint32_t at_end = 0, at_edge = 0, at_vertex = 0;
    for (uint32_t g = 0; g < n_graphs; ++g) {
        const uint32_t v0 = vertex_off[g], e0 = edge_off[g], ne = edge_off[g + 1] - e0;
        Graph G;
        G.nv = vertex_off[g + 1] - v0;
        G.k = k[g / n_regions];
        G.bases = bases;
        G.vbase = vertex_base + v0;
        G.src.assign(edge_src + e0, edge_src + e0 + ne), G.dst.assign(edge_dst + e0, edge_dst + e0 + ne);
        G.mult.assign(edge_mult + e0, edge_mult + e0 + ne), G.pmult.assign(edge_pmult + e0, edge_pmult + e0 + ne);
        G.is_ref.assign(edge_is_ref + e0, edge_is_ref + e0 + ne);
        G.gone.assign(ne, 0);
        for (uint32_t e = 0; e < ne; ++e) G.gone[e] = edge_absent && edge_absent[e0 + e], edge_removed[e0 + e] = 0;
        for (uint32_t v = 0; v < G.nv; ++v) G.count += !(vertex_absent && vertex_absent[v0 + v]);
        const uint32_t factor = prune_factor[g];
        uint32_t tally[4] = {0, 0, 0, 0};
        end_off[g] = at_end, new_edge_off[g] = at_edge, new_vertex_off[g] = at_vertex;
        for (uint32_t kind = 0; kind < 2; ++kind) {
            if (!(ops & (kind ? 2u : 1u))) continue;
            const bool tail = kind == 0;
            G.summaries();
            std::vector<uint32_t> todo;
            for (uint32_t v = 0; v < G.nvt(); ++v) {
                if (v < G.nv && vertex_absent && vertex_absent[v0 + v]) continue;
                if (tail ? G.dout[v] == 0 && !G.is_ref_sink(v) : G.din[v] == 0 && !G.is_ref_source(v)) todo.push_back(v);
            }
            std::vector<uint32_t> mark(G.nvt() + todo.size() * G.k + 1, 0);
            uint32_t stamp = 0;
            for (uint32_t vertex : todo) {
                ++stamp;
                if (mark.size() < G.nvt()) mark.resize(G.nvt(), 0);
                uint32_t status = NONE, v = vertex, steps = 0, made = NONE;
                std::vector<uint32_t> walk, alt_path, ref_path;
                std::vector<uint8_t> rs, as;
                Cigar c;
                for (;;) {
                    const bool done = tail ? G.din[v] != 1 || G.dout[v] >= 2 : G.is_ref_node(v) || G.dout[v] != 1;
                    if (done) break;
                    const uint32_t e = (tail ? G.in_edge[v] : G.out_edge[v]) - 1;
                    if (G.pmult[e] < factor) walk.clear();
                    else walk.push_back(v), mark[v] = stamp;
                    v = tail ? G.src[e] : G.dst[e];
                    if (mark[v] == stamp) { status = LOOP; break; }
                    if (++steps > G.nvt()) { status = REFERENCE_FAILS; break; }
                }
                if (status == NONE && !(tail ? G.dout[v] > 1 : G.is_ref_node(v))) status = NO_PATH;
                if (status == NONE) {
                    alt_path.push_back(v);
                    alt_path.insert(alt_path.end(), walk.rbegin(), walk.rend());
                    const int64_t min_len = tail ? std::max(1, min_dangling_branch_length) : min_dangling_branch_length;
                    if (tail ? G.is_ref_source(v) : G.is_ref_sink(v)) status = AT_REF_END;
                    else if ((int64_t)alt_path.size() < min_len + 1) status = TOO_SHORT;
                }
                if (status == NONE) {
                    const uint32_t bl = tail ? G.in_edge[alt_path[1]] - 1 : NONE;
                    for (uint32_t x = alt_path[0]; x != NONE;) {
                        if (ref_path.size() > G.nvt()) { status = REFERENCE_FAILS; break; }
                        ref_path.push_back(x);
                        if (tail) {
                            if (G.ref_out[x]) x = G.dst[G.ref_out[x] - 1];
                            else {
                                const bool mine = bl != NONE && G.src[bl] == x;
                                if (G.dout[x] - (mine ? 1u : 0u) != 1u) x = NONE;
                                else {
                                    uint32_t e = G.out_edge[x] - 1;
                                    if (mine && e == bl) e = G.out_min[x] - 1;
                                    x = G.dst[e];
                                }
                            }
                        } else {
                            x = G.prev_ref[x] ? G.src[G.prev_ref[x] - 1] : NONE;
                        }
                    }
                }
                if (status == NONE) {
                    for (int which = 0; which < 2; ++which) {
                        std::vector<uint8_t> &s = which ? as : rs;
                        for (uint32_t x : which ? alt_path : ref_path) {
                            if (!tail && G.din[x] == 0)
                                for (uint32_t t = 0; t < G.k; ++t) s.push_back(G.kb(x, G.k - 1 - t));
                            else
                                s.push_back(G.kb(x, G.k - 1));
                        }
                    }
                    c = align(rs, as, weights);
                    const uint32_t n_c = (uint32_t)c.el.size();
                    const auto op = [&](uint32_t i) { return c.el[i] & 15u; };
                    const auto len = [&](uint32_t i) { return (int64_t)(c.el[i] >> 4); };
                    const int64_t m = (int64_t)as.size(), n_ref = (int64_t)ref_path.size(), n_alt = (int64_t)alt_path.size();
                    bool changed = false;
                    if (!(n_c != 0 && n_c <= 3 && (tail ? op(n_c - 1) == OP_M : op(0) == OP_M))) {
                        status = CIGAR_NOT_OKAY;
                    } else if (tail) {
                        const int64_t last_ref_index = (int64_t)c.ref_len - 1;
                        int64_t suffix = m;
                        for (int64_t l = 1; l <= m; ++l)
                            if (last_ref_index - l + 1 < 0 || rs[last_ref_index - l + 1] != as[m - l]) { suffix = l - 1; break; }
                        suffix = std::min(suffix, len(n_c - 1));
                        const bool few = min_matching_bases >= 0 ? suffix < min_matching_bases : suffix == 0;
                        const int64_t alt_index = std::max<int64_t>(std::max<int64_t>((int64_t)c.read_len - suffix, 0) - 1, 0);
                        const bool leading = op(0) == OP_D && len(0) + suffix == last_ref_index + 1;
                        const int64_t ref_index = last_ref_index - suffix + 1 + (leading ? 1 : 0);
                        if (few) status = TOO_FEW_MATCHING;
                        else if (ref_index <= 0) status = WHOLE_INSERTION;
                        else if (ref_index >= n_ref || alt_index >= n_alt) status = REFERENCE_FAILS;
                        else made = G.add_edge(alt_path[alt_index], ref_path[ref_index], 1) - ne, status = MERGED, changed = true;
                    } else {
                        int64_t i0 = -1, i1 = -1;
                        if (min_matching_bases >= 0) {
                            int64_t ri = (int64_t)c.ref_len - 1, qi = m - 1;
                            bool stop = false;
                            for (int q = (int)n_c - 1; q >= 0 && !stop; --q) {
                                if (op(q) != OP_M) break;
                                for (int64_t j = 0; j < len(q); ++j) {
                                    if (rs[ri] != as[qi]) { stop = true; break; }
                                    --ri, --qi;
                                    if (ri < 0 || qi < 0) { stop = true; break; }
                                }
                            }
                            if (m - 1 - qi < min_matching_bases) status = TOO_FEW_MATCHING;
                            else if (ri <= 0 || qi <= 0) status = NO_MERGE_POINT;
                            else if (ri >= n_ref - 1) status = CANNOT_PUSH_REF;
                            i0 = ri, i1 = qi;
                        } else {
                            const int64_t max_index = len(0);
                            const int64_t max_mm = max_mismatches > 0 ? max_mismatches : std::max<int64_t>(1, max_index / G.k);
                            int64_t mm = 0, last_good = -1;
                            status = NO_MERGE_POINT;
                            for (int64_t i = 0; i < max_index; ++i)
                                if (rs[i] != as[i]) {
                                    if (++mm > max_mm) { status = TOO_MANY_MISMATCHES, last_good = -1; break; }
                                    last_good = i;
                                }
                            if (last_good >= 0) status = last_good >= n_ref - 1 ? CANNOT_PUSH_REF : NONE;
                            i0 = i1 = last_good;
                        }
                        if (status == NONE) {
                            const int64_t num = i1 - n_alt + 2;
                            if (i1 >= n_alt) {
                                const int64_t iref = n_alt - 1 + ((int64_t)c.ref_len - (int64_t)c.read_len) + num;
                                if (iref >= n_ref || iref < 0) {
                                    status = CANNOT_EXTEND;
                                } else {
                                    const uint32_t dsrc = alt_path.back(), ref_v = ref_path[iref];
                                    uint32_t se = NONE;
                                    for (uint32_t e = 0; e < G.src.size(); ++e)
                                        if (!G.gone[e] && G.src[e] == dsrc && (se == NONE || G.mult[e] > G.mult[se])) se = e;
                                    if (se == NONE) {
                                        status = REFERENCE_FAILS;
                                    } else {
                                        uint32_t prev_v = G.dst[se];
                                        const uint32_t multiplicity = G.mult[se];
                                        G.gone[se] = 1;
                                        if (se < ne) edge_removed[e0 + se] = 1;
                                        changed = true;
                                        alt_path.pop_back();
                                        for (int64_t i = num; i >= 1; --i) {
                                            std::vector<uint8_t> km(G.k);
                                            for (uint32_t t = 0; t < G.k; ++t) km[t] = i + t < num ? G.kb(ref_v, (uint32_t)(i + t)) : G.kb(dsrc, (uint32_t)(i + t - num));
                                            const uint32_t new_v = G.nvt();
                                            G.new_kmer.push_back(km);
                                            ++G.count;
                                            G.add_edge(new_v, prev_v, multiplicity);
                                            alt_path.push_back(new_v);
                                            prev_v = new_v;
                                        }
                                    }
                                }
                            }
                            if (status == NONE) made = G.add_edge(ref_path[i0 + 1], alt_path[i1], 1) - ne, status = MERGED, changed = true;
                        }
                    }
                    if (changed) G.summaries();
                }
                if (at_end >= capacity[0]) return 1;
                end_vertex[at_end] = vertex, end_kind[at_end] = kind, end_status[at_end] = status;
                end_alt_len[at_end] = (uint32_t)as.size(), end_ref_len[at_end] = (uint32_t)rs.size(), end_n_cigar[at_end] = (uint32_t)c.el.size();
                for (uint32_t i = 0; i < 4; ++i) end_cigar[4 * (size_t)at_end + i] = i < c.el.size() ? c.el[i] : 0;
                end_edge[at_end] = made;
                ++at_end;
                ++tally[2 * kind];
                tally[2 * kind + 1] += status == MERGED;
            }
        }
        const uint32_t n_new_e = (uint32_t)G.src.size() - ne, n_new_v = (uint32_t)G.new_kmer.size();
        if (at_edge + n_new_e > capacity[1] || at_vertex + n_new_v > capacity[2]) return 1;
        for (uint32_t i = 0; i < n_new_e; ++i) {
            const uint32_t e = ne + i;
            ne_src[at_edge + i] = G.gone[e] ? NONE : G.src[e], ne_dst[at_edge + i] = G.gone[e] ? NONE : G.dst[e];
            ne_mult[at_edge + i] = G.mult[e], ne_pmult[at_edge + i] = G.pmult[e];
        }
        for (uint32_t i = 0; i < n_new_v; ++i) {
            memset(new_kmer + (size_t)(at_vertex + i) * kmer_stride, 0, kmer_stride);
            memcpy(new_kmer + (size_t)(at_vertex + i) * kmer_stride, G.new_kmer[i].data(), G.k);
        }
        at_edge += n_new_e, at_vertex += n_new_v;
        const uint32_t vals[6] = {tally[0], tally[1], tally[2], tally[3], n_new_e, n_new_v};
        memcpy(counts + 6 * (size_t)g, vals, sizeof vals);
    }
    end_off[n_graphs] = at_end, new_edge_off[n_graphs] = at_edge, new_vertex_off[n_graphs] = at_vertex;
    return 0;
}
